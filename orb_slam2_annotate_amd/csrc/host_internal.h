// host_internal.h -- what one host translation unit of csrc/ defines for another.  The defining file and every user
// include it, so a signature that drifts is a compile error (the functions are extern "C": a hand-copied prototype would
// link whatever its parameters say).  tests/test_host_internal_header.py keeps prototypes out of the sources and dead
// entries out of this list.
#pragma once
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/orbfe.h"
#include "kernels.h"

namespace orbfe {
// extractor.hip: sets the text orbfe_last_error() returns on the calling thread; returns `code`
int fail(int code, const std::string& msg);
}  // namespace orbfe

extern "C" {
// ---- extractor.hip (struct orbfe_extractor lives there) ----
// a consumer of the last extract call's outputs on the handle's own stream: begin orders stream 0 behind every sub-batch
// and returns it, end marks the consumer's last kernel for the next extract call to wait for
int orbfe_extractor_consumer_begin_(orbfe_extractor* e, hipStream_t* s);
int orbfe_extractor_consumer_end_(orbfe_extractor* e);
// how the last extract call was split; streams / chunkDone: orbfe_extractor::kMaxStreams (32) entries
int orbfe_extractor_split_(orbfe_extractor* e, int* S, int* per, int* frames, int* lanes, hipStream_t* streams,
                           hipEvent_t* chunkDone);
// stage-timer marks for work another translation unit enqueues on a sub-batch stream
void orbfe_extractor_stage_mark_(orbfe_extractor* e, int stage, int sub, int isEnd, hipStream_t s, int frames);
// device pointers of frame `frame` of the handle's own output block (the host-buffer calls)
int orbfe_extractor_output_device_(orbfe_extractor* e, int frame, const orbfe_keypoint** d_kp, const uint8_t** d_desc,
                                   int* n, int* device);
// a frame build that reads the output block was enqueued on `s`: the next call that writes the block waits for it
int orbfe_extractor_reader_end_(orbfe_extractor* e, hipStream_t s);
// pyramid views + scale tables of the last extract call
int orbfe_stereo_views_(orbfe_extractor* e, int frame, orbfe::PyramidViews* pv, float* scale, float* invScale,
                        int* nlevels, int* device, const float** d_scaleTab);
// test hooks: hold back / query a stream
int orbfe_debug_stall_launch_(hipStream_t s, int usec);
int orbfe_debug_stream_idle_(hipStream_t s);
// ---- k_ingest.hip (struct orbfe_rectifier lives there) ----
// the rectification of a sub-batch on that sub-batch's own stream; d_src == NULL only queries w / h / device
int orbfe_remap_launch_(orbfe_rectifier* r, const uint8_t* d_src, int n_frames, int sw, int sh, int sstride,
                        size_t sFrame, uint8_t* d_dst, int dstride, size_t dFrame, hipStream_t stream, int* w, int* h,
                        int* device);
}
