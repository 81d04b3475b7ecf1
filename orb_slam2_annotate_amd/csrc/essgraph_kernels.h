// essgraph_kernels.h -- launchers of k_essgraph.hip: the passes of Optimizer::OptimizeEssentialGraph on the arrays of EssArgs
// (essgraph_math.h).  All on one stream, in the order essgraph.hip enqueues them; no kernel uses a floating-point atomic, a
// cooperative launch, a grid-wide barrier or a spin wait, and every sum has the order essgraph_math.h gives it.
#pragma once
#include <hip/hip_runtime.h>

#include "essgraph_math.h"
#include "match_kernels.h"

namespace orbfe {

constexpr int kEssThreads = 64;         // per-edge, per-vertex and per-point kernels: one wave per workgroup
constexpr int kEssFactorThreads = 256;  // the one workgroup of the factorisation and the substitutions

// once per call: the measurements and the chi2 at the inputs (a lane per edge)
void launch_ess_measure(hipStream_t s, const EssArgs& a);
// per iteration: linearise (a lane per active edge), assemble (a wave per block of H that has edges), the record (one wave)
void launch_ess_linearise(hipStream_t s, const EssArgs& a, int cur);
// per trial: L = H + lambda I and x = b (a lane per element), the factorisation with the two substitutions and the
// vertices' trials (one workgroup), the edges' chi2 at the trial (a lane per active edge), the record (one wave)
void launch_ess_trial(hipStream_t s, const EssArgs& a, int cur, double lambda);
// the solver on its own (orbfe_block_sparse_solve7): a.H, a.b -> a.x, a.rec->ok
void launch_ess_solve(hipStream_t s, const EssArgs& a);
// the tail: one lane per point.  table NULL: xw -> xwOut; else the positions of slot[] in the table, in place
void launch_ess_correct_points(hipStream_t s, const double* sim3, const double* sim3Out, int nPoints, const float* xw,
                               const int32_t* refVertex, float* xwOut, const MapPointsDevice* table, const int32_t* slot);
// the positions of slot[0 .. n) of a table (orbfe_mappoints_positions)
void launch_ess_read_positions(hipStream_t s, const MapPointsDevice& table, const int32_t* slot, int n, float* xw);

}  // namespace orbfe
