// lba_kernels.h -- launchers of k_lba.hip: the passes of Optimizer::LocalBundleAdjustment / BundleAdjustment on the arrays of
// LbaArgs (lba_math.h).  All on one stream, in the order lba.hip enqueues them; no kernel uses a floating-point atomic, a
// cooperative launch or a grid-wide barrier, and every sum has the order lba_math.h gives it.
#pragma once
#include <hip/hip_runtime.h>

#include "lba_math.h"
#include "match_kernels.h"

namespace orbfe {

constexpr int kLbaThreads = 64;        // per-point and per-edge kernels: one wave per workgroup
constexpr int kLbaSolveThreads = 256;  // the one workgroup of the dense solve
constexpr int kLbaSolveMaxPoses = 256;  // free poses of a call: a column of the reduced system (12 KB) sits in LDS

// per iteration: linearise (a thread per point), pose blocks (a wave per free pose), the record (one wave)
void launch_lba_linearise(hipStream_t s, const LbaArgs& a, int cur, int robust);
// per trial: Schur per point, Schur blocks and right-hand side (a wave each), the solve with the poses' trials (one
// workgroup), the points' trials with the errors-only pass (a thread per point), the record (one wave)
void launch_lba_trial(hipStream_t s, const LbaArgs& a, int cur, double lambda, int robust);
// after a round: first -> level[], final -> erase[]
void launch_lba_classify(hipStream_t s, const LbaArgs& a, int cur, int final, uint8_t* erase);
// the table form: positions from / to the resident map-point table
void launch_lba_gather(hipStream_t s, const LbaArgs& a, const MapPointsDevice& t, const int32_t* slot);
void launch_lba_scatter(hipStream_t s, const LbaArgs& a, int cur, const MapPointsDevice& t, const int32_t* slot);

}  // namespace orbfe
