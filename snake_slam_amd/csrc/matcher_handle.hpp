// The matcher / preprocess handle (shared by matcher.hip and preprocess.hip).
#pragma once
#include "common.hpp"
#include "stage.hpp"

struct snk_matcher : snk::HandleBase
{
    snk::DevBuf q, t, out, aux, aux2, cnt;
    // pinned staging of the per-frame (host pointer) projection matchers and of snk_pose_refine: the inputs of a call are copied here and
    // go up with one DMA, the results come back as one block (copies from / to pageable memory are staged by the runtime chunk by
    // chunk, and every one of them costs a submission: round 4, tools/latency_tracking.py)
    snk::HostBuf h_in, h_res;
    // device copy of the frame the projection matchers were last called with (track.hip): 1-2 coarse calls and one
    // fine call per frame (TrackingCoarse.cpp:234, TrackingFine.cpp:149) look at the same frame, which is uploaded once
    snk::DevBuf view;
    bool view_valid = false;  // snk_match_bind_frame: the arrays below live in `view`
    int view_n = 0, view_cols = 0, view_rows = 0;
    double view_bounds[4] = {0, 0, 0, 0};
    // sim3.hip: its[n], n = 0 .. sim3_its_cap, of snk_ransac_iterations under the parameters it was last filled with (the device-resident
    // registration RANSAC looks its iteration count up instead of evaluating log); pinned copy = the source of the upload
    snk::DevBuf sim3_its;
    snk::HostBuf sim3_its_host;
    int sim3_its_cap = -1, sim3_its_min = 0, sim3_its_max = 0;
    double sim3_its_probability = 0.0;
};

namespace snk
{
// Every host entry that takes host pointers stages a call the same way: the input arrays as one Block (stage.hpp) through a pinned
// buffer into a device buffer with one DMA, the results from a device buffer through a pinned buffer with one DMA back.  The forms
// that take a matcher alone use `h_in` -> `q` and `out` -> `h_res` (the map-side entries, pose, P3P, Sim3, kNN-2, the BoW matcher, the
// projection matchers); the general forms name the buffers (stereo and rectify keep their one block in `aux`, the grid answers from
// `aux2`, the filter reads `out` and answers from `aux`, snk_bow_transform has the vocabulary's own four buffers and stream).

// start[0 .. n]: begins at 0, never decreases
inline int check_starts(const int32_t* start, int n, const char* begin_msg, const char* order_msg)
{
    SNK_REQUIRE(start[0] == 0, begin_msg);
    for (int i = 0; i < n; ++i) SNK_REQUIRE(start[i + 1] >= start[i], order_msg);
    return SNK_OK;
}

// each buffer with what the call asks of it: the device sizes may carry an entry's slack, `res_bytes` is only what comes back
inline int stage_reserve(DevBuf& in, size_t in_dev_bytes, HostBuf& h_in, size_t in_bytes, DevBuf& out, size_t out_dev_bytes, HostBuf& h_res,
                         size_t res_bytes)
{
    int rc;
    if ((rc = in.reserve(in_dev_bytes)) != SNK_OK) return rc;
    if ((rc = out.reserve(out_dev_bytes)) != SNK_OK) return rc;
    if ((rc = h_in.reserve(in_bytes)) != SNK_OK) return rc;
    return h_res.reserve(res_bytes);
}
// `slack`: what an entry has always asked of `q` and `out` beyond its blocks
inline int stage_reserve(snk_matcher* m, size_t in_bytes, size_t out_bytes, size_t slack = 0)
{
    return stage_reserve(m->q, in_bytes + slack, m->h_in, in_bytes, m->out, out_bytes + slack, m->h_res, out_bytes);
}

// after stage_reserve: the parts into the pinned buffer, then the whole block to the device buffer
inline int stage_upload(const Block& in, HostBuf& h_in, DevBuf& dev, hipStream_t stream)
{
    in.copy(h_in.as<char>());
    SNK_HIP_CHECK(hipMemcpyAsync(dev.p, h_in.p, in.bytes, hipMemcpyHostToDevice, stream));
    return SNK_OK;
}
inline int stage_upload(snk_matcher* m, const Block& in)
{
    return stage_upload(in, m->h_in, m->q, m->stream);
}

// dev[offset .. offset + bytes) to h_res[host_offset ..); returns when it is there
inline int stage_download(HostBuf& h_res, size_t host_offset, const DevBuf& dev, size_t offset, size_t bytes, hipStream_t stream)
{
    SNK_HIP_CHECK(hipMemcpyAsync(h_res.as<char>() + host_offset, static_cast<const char*>(dev.p) + offset, bytes, hipMemcpyDeviceToHost, stream));
    SNK_HIP_CHECK(hipStreamSynchronize(stream));
    return SNK_OK;
}
// out[offset .. offset + bytes) to the same place of `h_res`
inline int stage_download(snk_matcher* m, size_t offset, size_t bytes)
{
    return stage_download(m->h_res, offset, m->out, offset, bytes, m->stream);
}

// snk_stereo_match_batch_dev with the option of doing Frame::allocateTmp's -1000 prefill of right_points / depth itself (the one-call front-end)
int stereo_match_batch_dev_impl(snk_matcher* m, const snk_kp64* left_dev, const uint64_t* desc_left_dev, const int32_t* nl_dev, int nl_cap,
                                const snk_kp64* right_dev, const uint64_t* desc_right_dev, const int32_t* nr_dev, int nr_cap, int batch, double bf,
                                const float* level_scale_host, int n_levels, int relaxed, float* right_points_dev, float* depth_dev,
                                int32_t* n_matches_dev, bool prefill);
// both rectifications of a stereo frame in one launch: image 0 of the pair (kps_dev[0 .. cap)) with rect_left (+ normalized points), image 1
// (kps_dev[cap .. 2 cap)) with rect_right; n_dev[2], out_dev[2][cap]
int rectify_pair_dev(snk_matcher* m, const snk_rectification* rect_left, const snk_rectification* rect_right, const snk_keypoint* kps_dev,
                     const int32_t* n_dev, int cap, snk_kp64* out_dev, double* normalized_left_dev);
}  // namespace snk
