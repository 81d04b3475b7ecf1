// window_call.h -- one call of the window-search machinery (matcher.hip: window_search_multi) as the entry points describe
// it: the jobs, what a claim job replays, and the producer that may write the jobs' queries on the device.  matcher.hip holds
// the machinery and the entry points on host arrays, mappoints_search.hip the producers and the entry points on the resident
// map points.
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "../../include/orbfe.h"
#include "arena.h"
#include "host_internal.h"
#include "match_kernels.h"

namespace orbfe {

struct WindowResult {
  std::vector<int32_t> count;
  std::vector<uint32_t> cand;  // [nq * K] (dist << 16 | feature index) in scan order
  int K = 0;
};

struct ClaimSpec {
  int mode = CLAIM_BEST, maxDist = 100, checkOri = 0;
  float nnratio = 0.0f;
  const uint8_t* blocked = nullptr;   // [f->n] features taken at entry (NULL: none)
  const uint8_t* blockVal = nullptr;  // [nq] does query i's match hide its feature (NULL: always; a producer may write it)
  const float* qAngle = nullptr;      // [nq] (checkOri)
  int32_t* match = nullptr;           // out: [f->n] (BEST / RATIO) or [nq] (INIT)
  int32_t* nMatches = nullptr;        // out
  float* prevX = nullptr;             // INIT, out [nq]: the matched feature's position, else the query's own
  float* prevY = nullptr;
  int rounds = 0;                     // out: rounds the fixed point took
};

// A prologue on the device-resident map points in front of the window search: ONE producer per call writes the queries of
// all the call's jobs on the device -- behind the call's one upload, from the map-point table -- so that only slot lists, masks,
// poses and level tables travel.  Job j searches part jobs[j].part of it.  The machinery reaches a producer through this
// interface alone; the four of them are mappoints_search.hip.
struct Producer {
  uint8_t* flagsOut = nullptr;        // host, out [total()] or NULL: the one flag array that travels back (which points project)
  QueryOut q{};                       // device: where launch() writes; carved by the machinery from the sizes below
  float* invSigma2 = nullptr;         // device: mvInvLevelSigma2 for a BEST job's chi-square gate; upload() sets it, or NULL
  virtual ~Producer() = default;
  // NULL when job mode (best: BEST, else the claim mode) may search a part of this producer, else what it needs instead
  virtual const char* accepts(bool best, int claimMode) const = 0;
  virtual int parts() const = 0;
  virtual int queries(int part) const = 0;   // windows of one part
  virtual size_t total() const = 0;          // windows of all parts: the length of every query array but desc
  virtual size_t desc_rows() const { return total(); }
  virtual bool with_obs() const { return false; }         // q.obs is written (a claim job's blockVal)
  virtual bool with_ur(bool stereo) const = 0;            // q.ur is written, for a job on a frame with / without u_right
  virtual hipError_t upload(Arena* a) = 0;                // region 1: the inputs, from a fresh state; up() alone
  virtual hipError_t launch(hipStream_t s) = 0;           // the prologue (and what must run ahead of it), writing q and the outputs
  virtual QueryOut part_queries(int part) const = 0;      // part's slice of q
  // the prologue alone: where launch() writes the projection itself, n4 arrays of 4-byte elements and the flags, [total()] each
  virtual void project_to(void* const* d4, uint8_t* flags) = 0;
};

// One window search = one frame + one set of query windows.  Several jobs of a call (Fuse against K neighbour key frames,
// the two directions of SearchBySim3) share ONE upload, one group of launches, one download and one synchronisation.
struct WindowJob {
  const orbfe_frame_view* f = nullptr;
  int nq = 0;
  const float *qx = nullptr, *qy = nullptr, *qr = nullptr;
  const int32_t *qmin = nullptr, *qmax = nullptr;
  const uint8_t* qactive = nullptr;
  const float* qur = nullptr;
  const uint8_t* qdesc = nullptr;  // jobs that pass the SAME pointer share one device copy
  // list mode (res != NULL): the counts and candidate lists come back
  WindowResult* res = nullptr;
  // BEST mode (bestOut != NULL): no candidate lists come back -- the device keeps the first minimum of every window, behind
  // Fuse's chi-square gate when gate != 0 (gur / invSigma2), and writes the keypoint or -1 (WindowQueries::best)
  int32_t* bestOut = nullptr;
  const float* gur = nullptr;
  const float* invSigma2 = nullptr;
  int nLevels = 0, gate = 0, maxDist = 256;
  // CLAIM mode (claim != NULL): the lists stay on the device and k_window_claim replays the reference's claim loop over
  // them (match_kernels.h: ClaimJob); the match array, the count and -- SearchForInitialization -- the updated previous
  // positions come back
  ClaimSpec* claim = nullptr;
  // behind a producer (all jobs of the call name the same one): the query arrays above are NULL, part `part` of it is searched
  Producer* producer = nullptr;
  int part = 0;
};

// Upload frames (unless resident) + queries or the producer's inputs, build the grids, search every window; grows K until
// every list fits.  K0: the first list capacity.
int window_search_multi(int device, WindowJob* jobs, int nJobs, int K0);
// A producer's prologue without a search (something to project, arguments checked, the table held): inputs up, its launch,
// the n4 + 1 projection arrays back in one copy; out4[i] (4-byte elements) and flags are [P.total()] or NULL: not wanted
int producer_run(int device, Producer& P, int n4, void* const* out4, uint8_t* flags);

bool frame_ok(const orbfe_frame_view* f);
// radius = th * scale_factors[level] and the level window [level + lo, level + hi] of each query
// (no_filter: no level filter at all, KeyFrame::GetFeaturesInArea, src/KeyFrame.cc:611-650)
int level_queries(const char* who, int n, const uint8_t* valid, const int32_t* level, const float* sf, int n_levels, float th, int lo,
                  int hi, bool no_filter, std::vector<float>* qr, std::vector<int32_t>* qmin, std::vector<int32_t>* qmax);
// The claim loops of the two searches that walk a frame's own map points, on the device (k_window_claim); shared by the
// host-array calls and the calls on the resident map points.
// SearchByProjection(CurrentFrame, LastFrame, th, bMono): claim loop :1572-1612 + rotation histogram :1614-1628
ClaimSpec last_frame_claim(const uint8_t* blocked, const uint8_t* obs_positive, const float* last_angle, int check_orientation,
                           int32_t* match_cur, int32_t* n_matches);
// SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist): claim loop :1726-1760
ClaimSpec keyframe_claim(const uint8_t* blocked, const float* kf_angle, int orb_dist, int check_orientation, int32_t* match_cur,
                         int32_t* n_matches);

}  // namespace orbfe
