// snake_hip.hpp — header-only C++17 adaptor over the C ABI (include/snake_hip.h) with the call
// shapes of the saiga classes Snake-SLAM uses on this path, so the Snake side changes types, not
// call sites.  Error style: the reference aborts through SAIGA_ASSERT /
// SAIGA_EXIT_ERROR (e.g. Snake/Preprocess/FeatureDetector.cpp:35); here every non-zero status
// becomes a std::runtime_error carrying snk_last_error().
#pragma once
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <stdexcept>
#include <string>
#include <tuple>
#include <type_traits>
#include <utility>
#include <vector>

#include "snake_hip.h"

namespace snake_hip
{
using DescriptorORB = std::array<uint64_t, 4>;  // Saiga::DescriptorORB (256 bit, trivially copyable)
using KeyPointF     = snk_keypoint;             // Saiga::KeyPoint<float>: point, size, angle, response, octave

inline void check(int rc, const char* what)
{
    if (rc != SNK_OK) throw std::runtime_error(std::string(what) + ": " + snk_last_error());
}

// Saiga::ORBExtractor / ORBExtractorGPU — Snake/Preprocess/FeatureDetector.cpp:31-41,119,124
class ORBExtractor
{
   public:
    ORBExtractor(int nfeatures, float scale_factor, int levels, int iniThFAST, int minThFAST, int /*threads*/ = 0,
                 int device = 0)
    {
        snk_orb_params p{nfeatures, scale_factor, levels, iniThFAST, minThFAST, 0};
        check(snk_orb_create(&p, device, nullptr, &h_), "snk_orb_create");
    }
    ~ORBExtractor() { snk_orb_destroy(h_); }
    ORBExtractor(const ORBExtractor&)            = delete;
    ORBExtractor& operator=(const ORBExtractor&) = delete;

    // Detect(ImageView<uchar>, vector<KeyPoint<float>>&, vector<DescriptorORB>&)
    void Detect(const uint8_t* data, int width, int height, int pitch_bytes, std::vector<KeyPointF>& keypoints,
                std::vector<DescriptorORB>& descriptors)
    {
        check(snk_orb_configure(h_, width, height, 1), "snk_orb_configure");
        int cap = 0;
        check(snk_orb_max_keypoints(h_, &cap), "snk_orb_max_keypoints");
        keypoints.resize((size_t)cap);
        descriptors.resize((size_t)cap);
        int n = 0;
        check(snk_orb_detect(h_, data, width, height, pitch_bytes, keypoints.data(),
                             reinterpret_cast<uint64_t(*)[4]>(descriptors.data()), cap, &n),
              "snk_orb_detect");
        keypoints.resize((size_t)n);
        descriptors.resize((size_t)n);
    }

   private:
    snk_orb* h_ = nullptr;
};

// Saiga::BruteForceMatcher<DescriptorORB> — Snake/Tracking/TrackingCoarse.cpp:350-352,373-387
class BruteForceMatcher
{
   public:
    explicit BruteForceMatcher(int device = 0) { check(snk_matcher_create(device, nullptr, &h_), "snk_matcher_create"); }
    ~BruteForceMatcher() { snk_matcher_destroy(h_); }
    BruteForceMatcher(const BruteForceMatcher&)            = delete;
    BruteForceMatcher& operator=(const BruteForceMatcher&) = delete;

    void matchKnn2(const std::vector<DescriptorORB>& d1, const std::vector<DescriptorORB>& d2)
    {
        knn_.resize(d1.size());
        check(snk_bf_knn2(h_, reinterpret_cast<const uint64_t(*)[4]>(d1.data()), (int)d1.size(),
                          reinterpret_cast<const uint64_t(*)[4]>(d2.data()), (int)d2.size(), knn_.data()),
              "snk_bf_knn2");
    }
    void matchKnn2_omp(const std::vector<DescriptorORB>& d1, const std::vector<DescriptorORB>& d2, int /*threads*/)
    {
        matchKnn2(d1, d2);
    }
    int filterMatches(int threshold, float ratio)
    {
        std::vector<std::array<int32_t, 2>> pairs(knn_.size() + 1);
        int n = 0;
        check(snk_bf_filter(h_, knn_.data(), (int)knn_.size(), threshold, ratio, reinterpret_cast<int32_t(*)[2]>(pairs.data()),
                            &n),
              "snk_bf_filter");
        matches.resize((size_t)n);
        for (int i = 0; i < n; ++i) matches[(size_t)i] = {pairs[(size_t)i][0], pairs[(size_t)i][1]};
        return n;
    }
    std::vector<std::pair<int, int>> matches;  // (index into d1, index into d2)
    const std::vector<snk_knn2>& knn() const { return knn_; }

   private:
    snk_matcher* h_ = nullptr;
    std::vector<snk_knn2> knn_;
};

// Snake::Preprocess::undistortKeypoints + StereoMatching — Snake/Preprocess/Preprocess.cpp:55-77,122-242
class Preprocess
{
   public:
    explicit Preprocess(int device = 0) { check(snk_matcher_create(device, nullptr, &h_), "snk_matcher_create"); }
    ~Preprocess() { snk_matcher_destroy(h_); }
    Preprocess(const Preprocess&)            = delete;
    Preprocess& operator=(const Preprocess&) = delete;

    // rect.Forward for every keypoint (angle / octave copied); normalized may be null
    void Rectify(const snk_rectification& rect, const std::vector<KeyPointF>& kps, std::vector<snk_kp64>& out,
                 std::vector<std::array<double, 2>>* normalized = nullptr)
    {
        out.resize(kps.size());
        if (normalized) normalized->resize(kps.size());
        check(snk_rectify(h_, &rect, kps.data(), (int)kps.size(), out.data(),
                          normalized ? reinterpret_cast<double(*)[2]>(normalized->data()) : nullptr),
              "snk_rectify");
    }

    // Preprocess::ComputeStereoFromRGBD (Preprocess.cpp:79-120): right_points / depth from the depth image; returns the match count.
    // Throws where the reference aborts (a keypoint outside the depth image, a depth outside [0, 20)).
    int ComputeStereoFromRGBD(const snk_rgbd_model& model, const std::vector<snk_kp64>& undistorted, const float* depth_image, int width,
                              int height, int pitch_floats, std::vector<float>& right_points, std::vector<float>& depth)
    {
        right_points.resize(undistorted.size());
        depth.resize(undistorted.size());
        int n = 0;
        check(snk_rgbd_stereo(h_, &model, undistorted.data(), (int)undistorted.size(), depth_image, width, height, pitch_floats,
                              right_points.data(), depth.data(), &n),
              "snk_rgbd_stereo");
        return n;
    }

    // returns the number of stereo matches; right_points / depth keep their -1000 fill where unmatched
    int StereoMatching(const std::vector<snk_kp64>& left_rectified, const std::vector<DescriptorORB>& desc_left,
                       const std::vector<snk_kp64>& right_rectified, const std::vector<DescriptorORB>& desc_right, double bf,
                       const std::vector<float>& level_scale, bool relaxed, std::vector<float>& right_points,
                       std::vector<float>& depth)
    {
        right_points.resize(left_rectified.size(), -1000.0f);
        depth.resize(left_rectified.size(), -1000.0f);
        int n = 0;
        check(snk_stereo_match(h_, left_rectified.data(), reinterpret_cast<const uint64_t(*)[4]>(desc_left.data()),
                               (int)left_rectified.size(), right_rectified.data(),
                               reinterpret_cast<const uint64_t(*)[4]>(desc_right.data()), (int)right_rectified.size(), bf,
                               level_scale.data(), (int)level_scale.size(), relaxed ? 1 : 0, right_points.data(),
                               depth.data(), &n),
              "snk_stereo_match");
        return n;
    }

   private:
    snk_matcher* h_ = nullptr;
};

// FeatureDetector::Detect (left + right) and Preprocess::Process for one frame in ONE call and one synchronisation
// (snk_frontend_process) -- Snake/Preprocess/FeatureDetector.cpp:116-156, Snake/Preprocess/Preprocess.cpp:35-53.  The result
// vectors hold what those two modules leave in Snake::Frame: left arrays in feature-grid order, right arrays in extractor order.
struct FrontendResult
{
    std::vector<KeyPointF> keypoints, keypoints_right;
    std::vector<DescriptorORB> descriptors, descriptors_right;
    std::vector<snk_kp64> undistorted_keypoints;
    std::vector<std::array<double, 2>> normalized_points;
    std::vector<int32_t> permutation, cell_start;
    std::vector<float> right_points, depth;
    int cols = 0, rows = 0, stereo_matches = 0;
};
class Frontend
{
   public:
    Frontend(const snk_frontend_params& p, int device = 0) : p_(p)
    {
        check(snk_frontend_create(&p, device, &h_), "snk_frontend_create");
        check(snk_frontend_grid_dims(h_, &cols_, &rows_), "snk_frontend_grid_dims");  // constants of the handle (the bounds / 20 px)
    }
    ~Frontend() { snk_frontend_destroy(h_); }
    Frontend(const Frontend&)            = delete;
    Frontend& operator=(const Frontend&) = delete;

    // right may be null for a mono handle; returns the number of stereo matches
    int Process(const uint8_t* left, int pitch_left, const uint8_t* right, int pitch_right, int width, int height, FrontendResult& r)
    {
        snk_frontend_frame f = bind(width, height, r);
        check(snk_frontend_process(h_, left, pitch_left, right, pitch_right, width, height, &f), "snk_frontend_process");
        return finish(f, r);
    }
    // The pipelined form: Submit returns as soon as the frame is enqueued (it blocks only while `depth` frames are uncollected, like
    // SynchronizedSlot::set of FeatureDetector::output_buffer, Snake/Preprocess/FeatureDetector.h:39); Collect hands out the oldest
    // frame, bit for bit what Process returns (SynchronizedSlot::get).  One thread may Submit while another Collects: the two share
    // nothing in this object (Collect sizes its arrays from what the C layer reports for the frame it is about to receive).
    void SetDepth(int depth) { check(snk_frontend_set_depth(h_, depth), "snk_frontend_set_depth"); }
    void Submit(const uint8_t* left, int pitch_left, const uint8_t* right, int pitch_right, int width, int height)
    {
        check(snk_frontend_submit(h_, left, pitch_left, right, pitch_right, width, height), "snk_frontend_submit");
    }
    // the images are page-locked memory of the caller (PinnedImage below) that stays untouched until the frame has been collected:
    // no staging copy (Snake/Preprocess/Input.h:48 -- the Input thread owns its image buffers)
    void SubmitPinned(const uint8_t* left, int pitch_left, const uint8_t* right, int pitch_right, int width, int height)
    {
        check(snk_frontend_submit_pinned(h_, left, pitch_left, right, pitch_right, width, height), "snk_frontend_submit_pinned");
    }
    int Collect(FrontendResult& r, int timeout_ms = -1)
    {
        int cap = 0;
        check(snk_frontend_peek(h_, timeout_ms, nullptr, nullptr, &cap), "snk_frontend_peek");  // blocks until a frame has been submitted
        snk_frontend_frame f = bind_capacity(cap, r);
        check(snk_frontend_collect(h_, &f, timeout_ms), "snk_frontend_collect");
        return finish(f, r);
    }
    int InFlight()
    {
        int n = 0;
        check(snk_frontend_in_flight(h_, &n), "snk_frontend_in_flight");
        return n;
    }
    const snk_frontend_params& params() const { return p_; }

   private:
    // result vectors at capacity, pointers into them (Process: the calling thread is the only user of the handle)
    snk_frontend_frame bind(int width, int height, FrontendResult& r)
    {
        if (cap_ == 0 || width != cap_w_ || height != cap_h_)
        {
            check(snk_frontend_max_keypoints(h_, width, height, &cap_), "snk_frontend_max_keypoints");
            cap_w_ = width, cap_h_ = height;
        }
        return bind_capacity(cap_, r);
    }
    snk_frontend_frame bind_capacity(int cap, FrontendResult& r) const
    {
        r.cols = cols_, r.rows = rows_;
        const size_t c = (size_t)cap;
        r.keypoints.resize(c), r.keypoints_right.resize(c), r.descriptors.resize(c), r.descriptors_right.resize(c);
        r.undistorted_keypoints.resize(c), r.normalized_points.resize(c), r.permutation.resize(c), r.right_points.resize(c), r.depth.resize(c);
        r.cell_start.resize((size_t)r.cols * r.rows + 1);
        snk_frontend_frame f{};
        f.capacity              = cap;
        f.keypoints             = r.keypoints.data();
        f.descriptors           = reinterpret_cast<uint64_t(*)[4]>(r.descriptors.data());
        f.undistorted_keypoints = r.undistorted_keypoints.data();
        f.normalized_points     = reinterpret_cast<double(*)[2]>(r.normalized_points.data());
        f.permutation           = r.permutation.data();
        f.cell_start            = r.cell_start.data();
        f.right_points          = r.right_points.data();
        f.depth                 = r.depth.data();
        f.keypoints_right       = r.keypoints_right.data();
        f.descriptors_right     = reinterpret_cast<uint64_t(*)[4]>(r.descriptors_right.data());
        return f;
    }
    static int finish(const snk_frontend_frame& f, FrontendResult& r)
    {
        const size_t n = (size_t)f.n, nr = (size_t)f.n_right;
        r.keypoints.resize(n), r.descriptors.resize(n), r.undistorted_keypoints.resize(n), r.normalized_points.resize(n);
        r.permutation.resize(n), r.right_points.resize(n), r.depth.resize(n);
        r.keypoints_right.resize(nr), r.descriptors_right.resize(nr);
        r.stereo_matches = f.n_stereo;
        return f.n_stereo;
    }
    snk_frontend* h_ = nullptr;
    snk_frontend_params p_;
    int cap_ = 0, cap_w_ = 0, cap_h_ = 0, cols_ = 0, rows_ = 0;  // cap_*: Process only; cols_ / rows_: set once in the constructor
};

// Page-locked image memory for Frontend::SubmitPinned (snk_pinned_alloc): what Snake's Input thread would allocate its image buffers from.
class PinnedImage
{
   public:
    PinnedImage(int pitch, int height, int count = 1) : pitch_(pitch), height_(height)
    {
        void* p = nullptr;
        check(snk_pinned_alloc((size_t)pitch * height * count, &p), "snk_pinned_alloc");
        p_ = static_cast<uint8_t*>(p);
    }
    ~PinnedImage() { snk_pinned_free(p_); }
    PinnedImage(const PinnedImage&)            = delete;
    PinnedImage& operator=(const PinnedImage&) = delete;
    uint8_t* data(int image = 0) { return p_ + (size_t)image * pitch_ * height_; }
    int pitch() const { return pitch_; }

   private:
    uint8_t* p_ = nullptr;
    int pitch_ = 0, height_ = 0;
};

// Frame data the tracking matchers read, grid-ordered (Snake/Map/Features.h:18-41, Frame.h:44-46).
struct FrameView
{
    std::vector<snk_kp64> undistorted_keypoints;
    std::vector<DescriptorORB> descriptors;
    std::vector<float> right_points;
    std::vector<uint8_t> taken;  // mvpMapPoints[i] != nullptr
    std::vector<int32_t> cell_start;
    int cols = 0, rows = 0;
    snk_grid_bounds bounds{};

    snk_frame_view view() const
    {
        snk_frame_view v{};
        v.n            = (int)undistorted_keypoints.size();
        v.cols         = cols;
        v.rows         = rows;
        v.kps          = undistorted_keypoints.data();
        v.desc         = reinterpret_cast<const uint64_t(*)[4]>(descriptors.data());
        v.right_points = right_points.data();
        v.taken        = taken.data();
        v.cell_start   = cell_start.data();
        v.bounds       = bounds;
        return v;
    }
};

// frame.grid.create(featureGridBounds, undistorted_keypoints) + the three SnakeORBMatcher searches
// (Snake/Preprocess/Preprocess.cpp:246; Snake/Tracking/SnakeORBMatcher.h:21-30)
class SnakeORBMatcher
{
   public:
    explicit SnakeORBMatcher(int device = 0) { check(snk_matcher_create(device, nullptr, &h_), "snk_matcher_create"); }
    ~SnakeORBMatcher() { snk_matcher_destroy(h_); }
    SnakeORBMatcher(const SnakeORBMatcher&)            = delete;
    SnakeORBMatcher& operator=(const SnakeORBMatcher&) = delete;

    // returns the permutation (new index of every feature); fills frame.cell_start / cols / rows
    std::vector<int32_t> CreateGrid(FrameView& frame, const snk_grid_bounds& bounds)
    {
        frame.bounds = bounds;
        const int n  = (int)frame.undistorted_keypoints.size();
        std::vector<int32_t> perm((size_t)n + 1);
        const int cols = std::max(1, (int)std::ceil((bounds.max_x - bounds.min_x) / 20.0));
        const int rows = std::max(1, (int)std::ceil((bounds.max_y - bounds.min_y) / 20.0));
        frame.cell_start.assign((size_t)cols * rows + 1, 0);
        check(snk_feature_grid(h_, frame.undistorted_keypoints.data(), n, &bounds, perm.data(), frame.cell_start.data(),
                               &frame.cols, &frame.rows),
              "snk_feature_grid");
        perm.resize((size_t)n);
        return perm;
    }
    // The Tracking thread makes 1-2 coarse calls and one fine call on the same frame: BindFrame uploads the frame once and returns
    // a TOKEN; the Search* overloads that take the token send nothing but the points.  The binding is explicit -- a FrameView
    // object that is refilled or re-created at the same address can never be mistaken for the frame on the device (round 2
    // compared addresses) -- and a token of an earlier binding is refused (std::logic_error).  After changing mvpMapPoints
    // (taken) between two calls: UpdateTaken(token, taken).  The Search* overloads that take a FrameView upload it, always.
    struct BoundFrame
    {
        uint64_t id = 0;
        int n       = 0;
    };
    BoundFrame BindFrame(const FrameView& frame)
    {
        const snk_frame_view v = frame.view();
        check(snk_match_bind_frame(h_, &v), "snk_match_bind_frame");
        bound_ = BoundFrame{++bind_counter_, v.n};
        return bound_;
    }
    void UpdateTaken(const BoundFrame& b, const std::vector<uint8_t>& taken)
    {
        require_bound(b);
        if ((int)taken.size() != b.n) throw std::invalid_argument("UpdateTaken: taken mask size differs from the bound frame's");
        check(snk_match_bound_taken(h_, taken.data()), "snk_match_bound_taken");
    }
    void UnbindFrame()
    {
        check(snk_match_bind_frame(h_, nullptr), "snk_match_bind_frame");
        bound_ = BoundFrame{};
    }

    // match[i] = feature index for local-map point i or -1; the caller sets mvpMapPoints[match[i]] = lm.points[i].mp
    int SearchByProjectionFrameFrame2(const FrameView& frame, const snk_camera& K, const double pose[7],
                                      const std::vector<snk_lm_coarse>& lm, float th, int featureError, int direction,
                                      const std::vector<float>& level_scale, std::vector<int32_t>& match)
    {
        const snk_frame_view v = frame.view();
        return coarse(&v, K, pose, lm, th, featureError, direction, level_scale, match);
    }
    int SearchByProjectionFrameFrame2(const BoundFrame& b, const snk_camera& K, const double pose[7],
                                      const std::vector<snk_lm_coarse>& lm, float th, int featureError, int direction,
                                      const std::vector<float>& level_scale, std::vector<int32_t>& match)
    {
        require_bound(b);
        return coarse(nullptr, K, pose, lm, th, featureError, direction, level_scale, match);
    }
    int SearchByProjection2(const FrameView& frame, const snk_camera& K, const double pose[7], std::vector<snk_lm_fine>& lm,
                            float th, float ratio, const std::vector<float>& level_scale, std::vector<int32_t>& match,
                            std::vector<uint8_t>& visible)
    {
        const snk_frame_view v = frame.view();
        return fine(&v, K, pose, lm, th, ratio, level_scale, match, visible);
    }
    int SearchByProjection2(const BoundFrame& b, const snk_camera& K, const double pose[7], std::vector<snk_lm_fine>& lm, float th,
                            float ratio, const std::vector<float>& level_scale, std::vector<int32_t>& match,
                            std::vector<uint8_t>& visible)
    {
        require_bound(b);
        return fine(nullptr, K, pose, lm, th, ratio, level_scale, match, visible);
    }
    int SearchByProjectionFrameToKeyframe(const FrameView& frame, const snk_camera& K, const double pose[7],
                                          const std::vector<std::array<double, 3>>& positions,
                                          const std::vector<DescriptorORB>& descriptors, const std::vector<uint8_t>& skip, float th,
                                          int featureError, std::vector<int32_t>& match)
    {
        const snk_frame_view v = frame.view();
        match.assign(positions.size() + 1, -1);
        int n = 0;
        check(snk_match_project_keyframe(h_, &v, &K, pose, reinterpret_cast<const double(*)[3]>(positions.data()),
                                         reinterpret_cast<const uint64_t(*)[4]>(descriptors.data()), skip.data(),
                                         (int)positions.size(), th, featureError, match.data(), &n),
              "snk_match_project_keyframe");
        match.resize(positions.size());
        return n;
    }

   private:
    void require_bound(const BoundFrame& b) const
    {
        if (b.id == 0 || b.id != bound_.id) throw std::logic_error("stale or empty frame binding (BindFrame again)");
    }
    int coarse(const snk_frame_view* v, const snk_camera& K, const double pose[7], const std::vector<snk_lm_coarse>& lm, float th,
               int featureError, int direction, const std::vector<float>& level_scale, std::vector<int32_t>& match)
    {
        match.assign(lm.size() + 1, -1);
        int n = 0;
        check(snk_match_project_coarse(h_, v, &K, pose, lm.data(), (int)lm.size(), th, featureError, direction, level_scale.data(),
                                       (int)level_scale.size(), match.data(), &n),
              "snk_match_project_coarse");
        match.resize(lm.size());
        return n;
    }
    int fine(const snk_frame_view* v, const snk_camera& K, const double pose[7], std::vector<snk_lm_fine>& lm, float th, float ratio,
             const std::vector<float>& level_scale, std::vector<int32_t>& match, std::vector<uint8_t>& visible)
    {
        match.assign(lm.size() + 1, -1);
        visible.assign(lm.size() + 1, 0);
        int n = 0;
        check(snk_match_project_fine(h_, v, &K, pose, lm.data(), (int)lm.size(), th, ratio, level_scale.data(),
                                     (int)level_scale.size(), match.data(), visible.data(), &n),
              "snk_match_project_fine");
        match.resize(lm.size());
        visible.resize(lm.size());
        return n;
    }
    snk_matcher* h_ = nullptr;
    BoundFrame bound_{};
    uint64_t bind_counter_ = 0;
};

// Snake::MappingORBMatcher (reference Snake/LocalMapping/MappingORBMatcher.h:15-45): the two keyframe-rate
// matchers that need no bag-of-words.  MapPoint / Keyframe pointers stay on the Snake side.
class MappingORBMatcher
{
   public:
    explicit MappingORBMatcher(int device = 0) { check(snk_matcher_create(device, nullptr, &h_), "snk_matcher_create"); }
    ~MappingORBMatcher() { snk_matcher_destroy(h_); }
    MappingORBMatcher(const MappingORBMatcher&)            = delete;
    MappingORBMatcher& operator=(const MappingORBMatcher&) = delete;

    // Fuse(kf, pose, point_mask, LocalMap<FusionPoint>, fuseCandidates, th, obs_factor, feature_th)
    // — MappingORBMatcher.cpp:359-480; kf_frame = kf->frame as a view, point_mask may be empty (= nullptr)
    int Fuse(const FrameView& kf_frame, const snk_camera& K, const double pose[7], const std::vector<uint8_t>& point_mask,
             const std::vector<snk_fusion_point>& points, std::vector<std::pair<int, int>>& fuseCandidates, float th,
             float obs_factor, int feature_th, const std::vector<float>& level_scale)
    {
        fuseCandidates.clear();
        if (!point_mask.empty() && point_mask.size() != points.size()) throw std::invalid_argument("point_mask size");
        const snk_frame_view v = kf_frame.view();
        std::vector<int32_t> best(points.size() + 1, -1);
        int n = 0;
        check(snk_match_fuse(h_, &v, &K, pose, points.data(), point_mask.empty() ? nullptr : point_mask.data(), (int)points.size(),
                             th, obs_factor, feature_th, level_scale.data(), (int)level_scale.size(), best.data(), &n),
              "snk_match_fuse");
        for (size_t i = 0; i < points.size(); ++i)
            if (best[i] >= 0) fuseCandidates.emplace_back(best[i], points[i].id);
        return n;
    }
    // SearchForTriangulationProject(grid, pose1, pose2, kf1, kf2, E12, vMatchedPairs, epipolarDistance,
    // featureDistance) — MappingORBMatcher.cpp:168-249; pairs are APPENDED like the reference does
    int SearchForTriangulationProject(const double* grid, int grid_rows, int grid_cols, const double pose1[7],
                                      const double pose2[7], const snk_camera& K, const std::vector<snk_kp64>& keypoints1,
                                      const std::vector<std::array<double, 2>>& normalized1,
                                      const std::vector<DescriptorORB>& descriptors1, const std::vector<uint8_t>& has_mp1,
                                      const FrameView& kf2_frame, const std::vector<std::array<double, 2>>& normalized2,
                                      const double E12[9], std::vector<std::pair<int, int>>& vMatchedPairs, float epipolarDistance,
                                      int featureDistance)
    {
        const snk_frame_view v = kf2_frame.view();
        std::vector<int32_t> match(keypoints1.size() + 1, -1);
        int n = 0;
        check(snk_match_triangulation_project(h_, grid, grid_rows, grid_cols, pose1, pose2, &K, keypoints1.data(),
                                              reinterpret_cast<const double(*)[2]>(normalized1.data()),
                                              reinterpret_cast<const uint64_t(*)[4]>(descriptors1.data()), has_mp1.data(),
                                              (int)keypoints1.size(), &v, reinterpret_cast<const double(*)[2]>(normalized2.data()),
                                              E12, epipolarDistance, featureDistance, match.data(), &n),
              "snk_match_triangulation_project");
        for (size_t i = 0; i < keypoints1.size(); ++i)
            if (match[i] >= 0) vMatchedPairs.emplace_back((int)i, match[i]);
        return n;
    }

    // frame->bow_feature_vec (std::map<node id, std::vector<feature index>>-like, ordered) flattened for the C ABI
    struct BowFeatureVector
    {
        std::vector<uint32_t> node_id;
        std::vector<int32_t> node_start{0}, features;
        template <typename Map>
        static BowFeatureVector from(const Map& fv)
        {
            BowFeatureVector b;
            for (const auto& node : fv)
            {
                b.node_id.push_back((uint32_t)node.first);
                for (auto f : node.second) b.features.push_back((int32_t)f);
                b.node_start.push_back((int32_t)b.features.size());
            }
            return b;
        }
        snk_bow_features view() const { return {(int32_t)node_id.size(), 0, node_id.data(), node_start.data(), features.data()}; }
    };
    // SearchForTriangulation2(kf1, kf2, E, vMatchedPairs, epipolarDistance, featureDistance) — MappingORBMatcher.cpp:14-99;
    // pairs are APPENDED in the reference's order
    int SearchForTriangulation2(const snk_camera& K, const double E[9], const std::vector<std::array<double, 2>>& normalized1,
                                const std::vector<DescriptorORB>& descriptors1, const std::vector<uint8_t>& has_mp1,
                                const BowFeatureVector& bow1, const std::vector<std::array<double, 2>>& normalized2,
                                const std::vector<DescriptorORB>& descriptors2, const std::vector<uint8_t>& has_mp2,
                                const BowFeatureVector& bow2, std::vector<std::pair<int, int>>& vMatchedPairs,
                                float epipolarDistance, int featureDistance)
    {
        const snk_bow_features b1 = bow1.view(), b2 = bow2.view();
        std::vector<std::array<int32_t, 2>> pairs(bow1.features.size() + 1);
        int n = 0;
        check(snk_match_triangulation_bow(h_, &K, E, reinterpret_cast<const double(*)[2]>(normalized1.data()),
                                          reinterpret_cast<const uint64_t(*)[4]>(descriptors1.data()), has_mp1.data(),
                                          (int)normalized1.size(), &b1, reinterpret_cast<const double(*)[2]>(normalized2.data()),
                                          reinterpret_cast<const uint64_t(*)[4]>(descriptors2.data()), has_mp2.data(),
                                          (int)normalized2.size(), &b2, epipolarDistance, featureDistance,
                                          reinterpret_cast<int32_t(*)[2]>(pairs.data()), &n),
              "snk_match_triangulation_bow");
        for (int i = 0; i < n; ++i) vMatchedPairs.emplace_back(pairs[i][0], pairs[i][1]);
        return n;
    }
    // SearchForTriangulationBF(pose1, pose2, kf1, kf2, E12, vMatchedPairs, epipolarDistance, featureDistance) —
    // MappingORBMatcher.cpp:102-165 (poses and epipolarDistance are unused there)
    int SearchForTriangulationBF(const snk_camera& K, const double E12[9], const std::vector<std::array<double, 2>>& normalized1,
                                 const std::vector<DescriptorORB>& descriptors1, const std::vector<uint8_t>& has_mp1,
                                 const std::vector<std::array<double, 2>>& normalized2,
                                 const std::vector<DescriptorORB>& descriptors2, const std::vector<uint8_t>& has_mp2,
                                 std::vector<std::pair<int, int>>& vMatchedPairs, int featureDistance)
    {
        std::vector<int32_t> match(normalized1.size() + 1, -1);
        int n = 0;
        check(snk_match_triangulation_bf(h_, &K, E12, reinterpret_cast<const double(*)[2]>(normalized1.data()),
                                         reinterpret_cast<const uint64_t(*)[4]>(descriptors1.data()), has_mp1.data(),
                                         (int)normalized1.size(), reinterpret_cast<const double(*)[2]>(normalized2.data()),
                                         reinterpret_cast<const uint64_t(*)[4]>(descriptors2.data()), has_mp2.data(),
                                         (int)normalized2.size(), featureDistance, match.data(), &n),
              "snk_match_triangulation_bf");
        for (size_t i = 0; i < normalized1.size(); ++i)
            if (match[i] >= 0) vMatchedPairs.emplace_back((int)i, match[i]);
        return n;
    }

   private:
    snk_matcher* h_ = nullptr;
};

// The per-observation search of Snake::DeferredMapper::Relink (reference Snake/Optimizer/DeferredMapper.cpp:39-165).
// The caller builds one query per feature i with a good map point (:61-64: position, descriptor, the descriptor of the
// point's first observation in another keyframe), calls RelinkSearch once, then applies the actions in feature order
// under map.LockFull() exactly as :75-163 do (ERASE / MOVE with the live GetMapPoint(best_idx) test).
class DeferredMapper
{
   public:
    static constexpr float relink_reprojection_error_threshold = 0.8f;  // :41
    static constexpr double relink_outlier_threshold           = 2.1;   // :42 reprojectionErrorThresholdMono
    static constexpr int relink_feature_threshold              = 25;    // :43
    explicit DeferredMapper(int device = 0) { check(snk_matcher_create(device, nullptr, &h_), "snk_matcher_create"); }
    ~DeferredMapper() { snk_matcher_destroy(h_); }
    DeferredMapper(const DeferredMapper&)            = delete;
    DeferredMapper& operator=(const DeferredMapper&) = delete;
    // returns the number of observations whose action is not SNK_RELINK_KEEP
    int RelinkSearch(const FrameView& kf_frame, const snk_camera& K, const double pose[7], const std::vector<snk_relink_query>& queries,
                     std::vector<int32_t>& action, std::vector<int32_t>& best_idx)
    {
        const snk_frame_view v = kf_frame.view();
        action.assign(queries.size() + 1, 0);
        best_idx.assign(queries.size() + 1, -1);
        int n = 0;
        check(snk_match_relink(h_, &v, &K, pose, queries.data(), (int)queries.size(), relink_reprojection_error_threshold,
                               relink_outlier_threshold, relink_feature_threshold, action.data(), best_idx.data(), &n),
              "snk_match_relink");
        action.resize(queries.size());
        best_idx.resize(queries.size());
        return n;
    }

   private:
    snk_matcher* h_ = nullptr;
};

// Snake::Triangulator (reference Snake/LocalMapping/Triangulator.h:23-87) from "pairs" to "points": the geometric loop of
// triangulate (Triangulator.cpp:127-157, :174-291) and the neighbour loop + first-wins test of Process (:42-47, :61-70),
// semantics "snk-tri v1".  The matchers that fill tmp_matches are MappingORBMatcher's (:164-171); the map edits of :72-106 stay
// on the Snake side, for the returned points with commit = 1, in order.
class Triangulator
{
   public:
    // TriangulationParams (Triangulator.h:27-38), the fields the geometric loop reads
    struct TriangulationParams
    {
        float errorMono   = 2.1f;
        float errorStereo = 2.3f;
    };
    // What the loop reads of one keyframe: kf->frame->undistorted_keypoints / right_points / depth, GetMapPoint(i) != nullptr,
    // kf->Pose() and (mono) kf->MedianDepth().  The vectors must outlive the call.
    struct KeyframeView
    {
        const std::vector<snk_kp64>* undistorted_keypoints = nullptr;
        const std::vector<float>* right_points             = nullptr;
        const std::vector<float>* depth                    = nullptr;
        const std::vector<uint8_t>* has_map_point          = nullptr;
        double pose[7]                                     = {0, 0, 0, 1, 0, 0, 0};
        float median_depth                                 = 0.f;
        snk_tri_view view() const
        {
            if (!undistorted_keypoints || !right_points || !depth || !has_map_point) throw std::invalid_argument("KeyframeView: unset array");
            const size_t n = undistorted_keypoints->size();
            if (right_points->size() != n || depth->size() != n || has_map_point->size() != n) throw std::invalid_argument("KeyframeView: array sizes");
            snk_tri_view v{};
            v.n            = (int32_t)n;
            v.kps          = undistorted_keypoints->data();
            v.right_points = right_points->data();
            v.depth        = depth->data();
            v.has_mp       = has_map_point->data();
            std::memcpy(v.pose, pose, sizeof(v.pose));
            return v;
        }
    };
    // ImageTriangulationResult (Triangulator.h:41-55) without the Keyframe pointers
    struct ImageTriangulationResult
    {
        std::vector<snk_new_point> newPoints;
    };

    // K, stereo_cam.bf, scalePyramid (level scales; Factor() = level_scale[1] / level_scale[0]), the global th_depth and
    // settings.inputType == InputType::Mono
    Triangulator(const snk_camera& K, const std::vector<float>& level_scale, double th_depth, bool mono, int device = 0)
        : K_(K), level_scale_(level_scale), th_depth_(th_depth), mono_(mono)
    {
        if (level_scale_.empty()) throw std::invalid_argument("level_scale is empty");
        check(snk_matcher_create(device, nullptr, &h_), "snk_matcher_create");
    }
    ~Triangulator() { snk_matcher_destroy(h_); }
    Triangulator(const Triangulator&)            = delete;
    Triangulator& operator=(const Triangulator&) = delete;

    // triangulate(params, kf1, kf2, precise) — Triangulator.cpp:113-294 — after the matchers: tmp_matches in, result.newPoints out
    ImageTriangulationResult triangulate(const TriangulationParams& params, const KeyframeView& kf1, const KeyframeView& kf2,
                                         const std::vector<std::pair<int, int>>& tmp_matches)
    {
        const snk_tri_params p = tri_params(params);
        const snk_tri_view v1 = kf1.view(), v2 = kf2.view();
        std::vector<int32_t> flat = flatten(tmp_matches);
        ImageTriangulationResult result;
        result.newPoints.resize(tmp_matches.size() + 1);
        int n = 0;
        check(snk_triangulate_pairs(h_, &K_, &p, &v1, &v2, kf2.median_depth, reinterpret_cast<const int32_t(*)[2]>(flat.data()),
                                    (int)tmp_matches.size(), level_scale_.data(), (int)level_scale_.size(), result.newPoints.data(), &n),
              "snk_triangulate_pairs");
        result.newPoints.resize((size_t)n);
        return result;
    }

    // Process(params, kf, out_points) — Triangulator.cpp:15-111 — from the matched pairs of every neighbour (tmp_keyframes order)
    // to newPointsa with the test of :67 already made: newPointsa[k].newPoints[j].commit == 1 <=> the loop of :61-108 creates a
    // map point for that entry.  Returns nnew (:106), the number of such entries.
    int Process(const TriangulationParams& params, const KeyframeView& kf, const std::vector<KeyframeView>& tmp_keyframes,
                const std::vector<std::vector<std::pair<int, int>>>& matches, std::vector<ImageTriangulationResult>& newPointsa)
    {
        if (matches.size() != tmp_keyframes.size()) throw std::invalid_argument("one match list per neighbour keyframe");
        const snk_tri_params p = tri_params(params);
        const snk_tri_view v1  = kf.view();
        std::vector<snk_tri_view> v2;
        std::vector<float> median;
        std::vector<int32_t> start{0}, flat;
        for (size_t k = 0; k < tmp_keyframes.size(); ++k)
        {
            v2.push_back(tmp_keyframes[k].view());
            median.push_back(tmp_keyframes[k].median_depth);
            const std::vector<int32_t> f = flatten(matches[k]);
            flat.insert(flat.end(), f.begin(), f.end());
            start.push_back((int32_t)(flat.size() / 2));
        }
        std::vector<snk_new_point> out(flat.size() / 2 + 1);
        std::vector<int32_t> out_start(tmp_keyframes.size() + 1, 0);
        int n = 0;
        check(snk_triangulate_neighbours(h_, &K_, &p, &v1, v2.data(), median.data(), (int)tmp_keyframes.size(),
                                         reinterpret_cast<const int32_t(*)[2]>(flat.data()), start.data(), level_scale_.data(),
                                         (int)level_scale_.size(), out.data(), out_start.data(), &n),
              "snk_triangulate_neighbours");
        newPointsa.assign(tmp_keyframes.size(), ImageTriangulationResult{});
        int nnew = 0;
        for (size_t k = 0; k < tmp_keyframes.size(); ++k)
        {
            newPointsa[k].newPoints.assign(out.begin() + out_start[k], out.begin() + out_start[k + 1]);
            for (const snk_new_point& np : newPointsa[k].newPoints) nnew += np.commit;
        }
        return nnew;
    }

   private:
    snk_tri_params tri_params(const TriangulationParams& params) const
    {
        snk_tri_params p{};
        p.error_mono   = params.errorMono;
        p.error_stereo = params.errorStereo;
        p.th_depth     = th_depth_;
        p.scale_factor = level_scale_.size() > 1 ? level_scale_[1] / level_scale_[0] : 1.2f;
        p.mono         = mono_ ? 1 : 0;
        return p;
    }
    static std::vector<int32_t> flatten(const std::vector<std::pair<int, int>>& m)
    {
        std::vector<int32_t> f;
        f.reserve(2 * m.size());
        for (const auto& [a, b] : m)
        {
            f.push_back(a);
            f.push_back(b);
        }
        return f;
    }
    snk_matcher* h_ = nullptr;
    snk_camera K_;
    std::vector<float> level_scale_;
    double th_depth_;
    bool mono_;
};

// MapPoint::ComputeDistinctiveDescriptors / UpdateNormal / UpdateDepth (reference Snake/Map/MapPoint.cpp:60-81, :120-135, :154-166)
// for a batch of points, semantics "snk-mp v1": the loops that call them per point (Triangulator.cpp:94-97, LocalMapping.cpp:179,215,
// NeighbourSearch.cpp:218-219, LocalBundleAdjustment.cpp:497, GlobalBundleAdjustment.cpp:502, ...) collect a PointView per point and
// make one call after the loop.  The list surgery (AddObservation, Replace, SetBadFlag) stays on the Snake side.
class MapPointRefresher
{
   public:
    // one entry of mObservations: obs.first->Pose(), obs.first->frame->descriptors[obs.second],
    // undistorted_keypoints[obs.second].octave, !obs.first->isBad().  The pose and the descriptor must outlive the call.
    struct Observation
    {
        const double* pose               = nullptr;  // qx qy qz qw tx ty tz
        const DescriptorORB* descriptor  = nullptr;
        int octave                       = 0;
        bool valid                       = true;
    };
    struct PointView
    {
        std::vector<Observation> observations;  // in the order of mObservations
        double position[3] = {0, 0, 0};
        int ref_obs        = -1;  // indexInternal(referenceKF) as an index into observations; -1: UpdateDepth leaves the point alone
    };

    explicit MapPointRefresher(int rule = SNK_MP_MEDIAN, int device = 0) : rule_(rule) { check(snk_matcher_create(device, nullptr, &h_), "snk_matcher_create"); }
    ~MapPointRefresher() { snk_matcher_destroy(h_); }
    MapPointRefresher(const MapPointRefresher&)            = delete;
    MapPointRefresher& operator=(const MapPointRefresher&) = delete;

    // the three updates of every point in one call; result[p].best = -1 leaves the descriptor as it was (MapPoint.cpp:75)
    std::vector<snk_mp_result> Refresh(const std::vector<PointView>& points, int what = SNK_MP_DESCRIPTOR | SNK_MP_NORMAL | SNK_MP_DEPTH)
    {
        std::vector<int32_t> start{0}, octave, ref;
        std::vector<DescriptorORB> desc;
        std::vector<std::array<double, 7>> pose;
        std::vector<std::array<double, 3>> position;
        std::vector<uint8_t> valid;
        for (const PointView& p : points)
        {
            for (const Observation& o : p.observations)
            {
                if (!o.pose || !o.descriptor) throw std::invalid_argument("MapPointRefresher: observation without pose / descriptor");
                std::array<double, 7> q;
                std::memcpy(q.data(), o.pose, sizeof(q));
                pose.push_back(q);
                desc.push_back(*o.descriptor);
                octave.push_back(o.octave);
                valid.push_back(o.valid ? 1 : 0);
            }
            start.push_back((int32_t)desc.size());
            position.push_back({p.position[0], p.position[1], p.position[2]});
            ref.push_back(p.ref_obs);
        }
        std::vector<snk_mp_result> out(points.size());
        const snk_mp_params par{rule_, what};
        check(snk_mappoint_refresh(h_, &par, (int)points.size(), start.data(), reinterpret_cast<const uint64_t(*)[4]>(desc.data()),
                                   reinterpret_cast<const double(*)[7]>(pose.data()), octave.data(), valid.data(),
                                   reinterpret_cast<const double(*)[3]>(position.data()), ref.data(), out.data()),
              "snk_mappoint_refresh");
        return out;
    }
    // after a replacement only the descriptor is wanted (MapPoint.cpp:244), after BA only the normal (LocalBundleAdjustment.cpp:497)
    std::vector<snk_mp_result> ComputeDistinctiveDescriptors(const std::vector<PointView>& points) { return Refresh(points, SNK_MP_DESCRIPTOR); }
    std::vector<snk_mp_result> UpdateNormal(const std::vector<PointView>& points) { return Refresh(points, SNK_MP_NORMAL); }
    std::vector<snk_mp_result> UpdateDepth(const std::vector<PointView>& points) { return Refresh(points, SNK_MP_DEPTH); }

   private:
    snk_matcher* h_ = nullptr;
    int rule_;
};

// Keyframe::UpdateConnections (reference Snake/Map/Keyframe.cpp:89-171) for a list of keyframes and the vote at the head of
// Tracking::UpdateLocalKeyFrames2 (Snake/Tracking/TrackingFine.cpp:230-268) for a list of frames, semantics "snk-covis v1": the
// caller flattens the map into a MapTables (keyframe slots and point ids are indices into it), makes one call and applies the lists:
// AddConnection(this, w) on every listed keyframe (Keyframe.cpp:150,157), connections = the list (:164), parent = list.Best() (:168).
class CovisibilityGraph
{
   public:
    struct MapTables
    {
        std::vector<uint8_t> kf_bad;                 // Keyframe::isBad()
        std::vector<int32_t> obs_start{0};           // per point, into obs
        std::vector<std::array<int32_t, 2>> obs;     // mp->GetObservationList() in list order: (keyframe slot, feature)
        std::vector<uint8_t> pt_flags;               // SNK_COVIS_PT_BAD | SNK_COVIS_PT_FAR
        std::vector<int32_t> feat_start{0};          // per keyframe, into feat_point / feat_depth
        std::vector<int32_t> feat_point;             // observations[i] as a point id, -1: none
        std::vector<float> feat_depth;               // frame->depth[i]

        // the next point id: its flags and its observation list
        int AddPoint(bool bad, bool far_stereo_point, const std::vector<std::pair<int, int>>& observations)
        {
            for (const auto& o : observations) obs.push_back({(int32_t)o.first, (int32_t)o.second});
            obs_start.push_back((int32_t)obs.size());
            pt_flags.push_back((uint8_t)((bad ? SNK_COVIS_PT_BAD : 0) | (far_stereo_point ? SNK_COVIS_PT_FAR : 0)));
            return (int)pt_flags.size() - 1;
        }
        // the next keyframe slot: its features in feature order
        int AddKeyframe(bool bad, const std::vector<int32_t>& points, const std::vector<float>& depth)
        {
            if (points.size() != depth.size()) throw std::invalid_argument("CovisibilityGraph: a depth per feature");
            feat_point.insert(feat_point.end(), points.begin(), points.end());
            feat_depth.insert(feat_depth.end(), depth.begin(), depth.end());
            feat_start.push_back((int32_t)feat_point.size());
            kf_bad.push_back(bad ? 1 : 0);
            return (int)kf_bad.size() - 1;
        }
        snk_covis_map view() const
        {
            snk_covis_map m;
            m.n_kf      = (int32_t)kf_bad.size();
            m.n_points  = (int32_t)pt_flags.size();
            m.n_obs     = (int32_t)obs.size();
            m.kf_bad    = kf_bad.data();
            m.obs_start = obs_start.data();
            m.obs       = reinterpret_cast<const int32_t(*)[2]>(obs.data());
            m.pt_flags  = pt_flags.data();
            return m;
        }
    };

    // one returned list: the last min(n_found, cap) entries of it, ascending by (weight, kf)
    struct List
    {
        std::vector<snk_covis_conn> connections;
        int n_found = 0;
        int status  = SNK_COVIS_OK;  // SNK_COVIS_UNCHANGED: leave the old connections (Keyframe.cpp:125-129)

        int Best() const { return connections.empty() ? -1 : connections.back().kf; }  // Keyframe.cpp:168, TrackingFine.cpp:268
        // KeyframeGraph::GetBestCovisibilityKeyFrames(N), KeyframeGraph.cpp:49-63: the last N, the best last
        std::vector<int> BestCovisibility(int N) const
        {
            N = std::max(0, std::min(N, (int)connections.size()));
            std::vector<int> v;
            for (size_t i = connections.size() - (size_t)N; i < connections.size(); ++i) v.push_back(connections[i].kf);
            return v;
        }
        // KeyframeGraph::GetCovisiblesByWeight(w), KeyframeGraph.cpp:148-172
        std::vector<int> CovisiblesByWeight(int w) const
        {
            std::vector<int> v;
            for (const snk_covis_conn& c : connections)
                if (c.weight >= w) v.push_back(c.kf);
            return v;
        }
    };

    explicit CovisibilityGraph(int th = 15, float th_depth = 40.0f, int cap = 256, int device = 0) : par_{th, th_depth, cap}
    {
        check(snk_matcher_create(device, nullptr, &h_), "snk_matcher_create");
    }
    ~CovisibilityGraph() { snk_matcher_destroy(h_); }
    CovisibilityGraph(const CovisibilityGraph&)            = delete;
    CovisibilityGraph& operator=(const CovisibilityGraph&) = delete;

    // Keyframe::UpdateConnections for every keyframe of `queries`, all against the same tables
    std::vector<List> UpdateConnections(const MapTables& map, const std::vector<int32_t>& queries)
    {
        const snk_covis_map m = map.view();
        std::vector<snk_covis_conn> conn(queries.size() * (size_t)par_.cap);
        std::vector<snk_covis_result> res(queries.size());
        check(snk_covis_update(h_, &m, map.feat_start.data(), map.feat_point.data(), map.feat_depth.data(), &par_, (int)queries.size(), queries.data(),
                               conn.data(), res.data()),
              "snk_covis_update");
        return lists(conn, res);
    }

    // the vote of UpdateLocalKeyFrames2 for every frame: frames[f] = its mvpMapPoints as point ids, -1: none; Best() = reference_keyframe
    std::vector<List> VoteLocalKeyframes(const MapTables& map, const std::vector<std::vector<int32_t>>& frames)
    {
        const snk_covis_map m = map.view();
        std::vector<int32_t> start{0}, point;
        for (const auto& f : frames)
        {
            point.insert(point.end(), f.begin(), f.end());
            start.push_back((int32_t)point.size());
        }
        std::vector<snk_covis_conn> conn(frames.size() * (size_t)par_.cap);
        std::vector<snk_covis_result> res(frames.size());
        check(snk_covis_vote(h_, &m, (int)frames.size(), start.data(), point.data(), &par_, conn.data(), res.data()), "snk_covis_vote");
        return lists(conn, res);
    }

   private:
    std::vector<List> lists(const std::vector<snk_covis_conn>& conn, const std::vector<snk_covis_result>& res) const
    {
        std::vector<List> out(res.size());
        for (size_t s = 0; s < res.size(); ++s)
        {
            const snk_covis_conn* row = conn.data() + s * (size_t)par_.cap;
            out[s].connections.assign(row, row + res[s].n_conn);
            out[s].n_found = res[s].n_found;
            out[s].status  = res[s].status;
        }
        return out;
    }
    snk_matcher* h_ = nullptr;
    snk_covis_params par_;
};

// The local map of fine tracking, semantics "snk-lmap v1": Select is the rest of Tracking::UpdateLocalKeyFrames2 behind the vote
// (reference Snake/Tracking/TrackingFine.cpp:272-323), Gather is Tracking::UpdateLocalPoints with LocalMap::addPoint (:328-356,
// Snake/Map/LocalMap.h:139-154), both for a list of frames.  The caller passes the vote's lists (CovisibilityGraph::VoteLocalKeyframes),
// every keyframe's connections and the map as tables, and sets lm.points from Frame::points / ::ids:
// mvpMapPoints[idx] = the MapPoint of ids[i].  The device forms run on arrays that are already in HBM and feed
// snk_match_project_fine_batch_dev directly.
class LocalMapBuilder
{
   public:
    struct Graph  // every keyframe's connections, ascending by (weight, kf): KeyframeGraph.cpp:124
    {
        std::vector<uint8_t> kf_bad;
        std::vector<int32_t> conn_start{0};
        std::vector<snk_covis_conn> conn_list;
        int AddKeyframe(bool bad, const std::vector<snk_covis_conn>& connections)
        {
            conn_list.insert(conn_list.end(), connections.begin(), connections.end());
            conn_start.push_back((int32_t)conn_list.size());
            kf_bad.push_back(bad ? 1 : 0);
            return (int)kf_bad.size() - 1;
        }
    };
    struct Points  // the keyframe side of the map and what FineTrackingPoint copies (LocalMap.h:46-53), a row per point id
    {
        std::vector<int32_t> feat_start{0}, feat_point;  // GetMapPointMatches() per keyframe slot as point ids, -1: none
        std::vector<uint8_t> pt_flags;                   // SNK_COVIS_PT_BAD
        std::vector<int32_t> pt_last_seen;               // MapPoint::lastFrameSeen
        std::vector<double> pos, normal;                 // [n][3]
        std::vector<uint64_t> desc;                      // [n][4]
        std::vector<float> ref_depth;
        std::vector<int32_t> ref_level;
        snk_lmap_map map() const
        {
            return snk_lmap_map{(int32_t)feat_start.size() - 1, (int32_t)pt_flags.size(), (int32_t)feat_point.size(), feat_start.data(), feat_point.data(),
                                pt_flags.data(), pt_last_seen.data()};
        }
        snk_lmap_points table() const { return snk_lmap_points{pos.data(), normal.data(), desc.data(), ref_depth.data(), ref_level.data()}; }
    };
    struct Selection  // [n_sets][kf_cap] local keyframes (-1 past n_local) and a record per set
    {
        std::vector<int32_t> local_kf;
        std::vector<snk_lmap_select_result> result;
    };
    struct Frame  // one frame's local map: points[i] belongs to the map point ids[i]
    {
        std::vector<snk_lm_fine> points;
        std::vector<int32_t> ids;
        snk_lmap_gather_result result{};
    };

    explicit LocalMapBuilder(const snk_lmap_params& params, int device = 0) : par_(params)
    {
        check(snk_matcher_create(device, nullptr, &h_), "snk_matcher_create");
    }
    ~LocalMapBuilder() { snk_matcher_destroy(h_); }
    LocalMapBuilder(const LocalMapBuilder&)            = delete;
    LocalMapBuilder& operator=(const LocalMapBuilder&) = delete;

    // votes[s] / frame_id[s]: the list of frame s as VoteLocalKeyframes returned it
    Selection Select(const std::vector<CovisibilityGraph::List>& votes, const Graph& graph, const std::vector<int32_t>& frame_id)
    {
        if (votes.size() != frame_id.size()) throw std::invalid_argument("LocalMapBuilder: a frame id per vote");
        size_t cap = 1;
        for (const auto& v : votes) cap = std::max(cap, v.connections.size());
        std::vector<snk_covis_conn> conn(votes.size() * cap, snk_covis_conn{-1, -1});
        std::vector<snk_covis_result> res(votes.size());
        for (size_t s = 0; s < votes.size(); ++s)
        {
            std::copy(votes[s].connections.begin(), votes[s].connections.end(), conn.begin() + (std::ptrdiff_t)(s * cap));
            res[s] = snk_covis_result{votes[s].n_found, (int32_t)votes[s].connections.size(), votes[s].Best(), votes[s].status};
        }
        Selection out;
        out.local_kf.assign(votes.size() * (size_t)par_.kf_cap, -1);
        out.result.resize(votes.size());
        check(snk_lmap_select(h_, (int)votes.size(), conn.data(), (int)cap, res.data(), (int)graph.kf_bad.size(), graph.kf_bad.data(), graph.conn_start.data(),
                              graph.conn_list.data(), frame_id.data(), &par_, out.local_kf.data(), out.result.data()),
              "snk_lmap_select");
        return out;
    }

    // own[s]: frame s's mvpMapPoints as point ids, -1: none
    std::vector<Frame> Gather(const Points& pts, const Selection& sel, const std::vector<int32_t>& frame_id, const std::vector<std::vector<int32_t>>& own,
                              int pts_cap)
    {
        const size_t n = sel.result.size();
        if (own.size() != n || frame_id.size() != n) throw std::invalid_argument("LocalMapBuilder: a frame id and a point list per set");
        std::vector<int32_t> start{0}, point;
        for (const auto& f : own)
        {
            point.insert(point.end(), f.begin(), f.end());
            start.push_back((int32_t)point.size());
        }
        const snk_lmap_map m      = pts.map();
        const snk_lmap_points tab = pts.table();
        std::vector<snk_lm_fine> lm(n * (size_t)std::max(pts_cap, 1));
        std::vector<int32_t> ids(n * (size_t)std::max(pts_cap, 1), -1), n_pts(n);
        std::vector<snk_lmap_gather_result> res(n);
        check(snk_lmap_gather(h_, (int)n, &m, &tab, frame_id.data(), sel.local_kf.data(), par_.kf_cap, sel.result.data(), start.data(), point.data(), pts_cap,
                              lm.data(), ids.data(), n_pts.data(), res.data()),
              "snk_lmap_gather");
        std::vector<Frame> out(n);
        for (size_t s = 0; s < n; ++s)
        {
            out[s].points.assign(lm.begin() + (std::ptrdiff_t)(s * (size_t)pts_cap), lm.begin() + (std::ptrdiff_t)(s * (size_t)pts_cap + (size_t)n_pts[s]));
            out[s].ids.assign(ids.begin() + (std::ptrdiff_t)(s * (size_t)pts_cap), ids.begin() + (std::ptrdiff_t)(s * (size_t)pts_cap + (size_t)n_pts[s]));
            out[s].result = res[s];
        }
        return out;
    }

    // the device forms: every pointer is device memory, nothing is copied, the call returns before the kernel has run
    void SelectDev(int n_sets, const snk_covis_conn* conn_dev, int vote_cap, const snk_covis_result* vote_dev, int n_kf, const uint8_t* kf_bad_dev,
                   const int32_t* conn_start_dev, int n_list, const snk_covis_conn* conn_list_dev, const int32_t* frame_id_dev, int32_t* local_kf_dev,
                   snk_lmap_select_result* out_dev)
    {
        check(snk_lmap_select_batch_dev(h_, n_sets, conn_dev, vote_cap, vote_dev, n_kf, kf_bad_dev, conn_start_dev, n_list, conn_list_dev, frame_id_dev, &par_,
                                        local_kf_dev, out_dev),
              "snk_lmap_select_batch_dev");
    }
    void GatherDev(int n_sets, const snk_lmap_map& map_dev, const snk_lmap_points& points_dev, const int32_t* frame_id_dev, const int32_t* local_kf_dev,
                   const snk_lmap_select_result* sel_dev, const int32_t* set_start_dev, int n_set_points, const int32_t* set_point_dev, int pts_cap,
                   snk_lm_fine* lm_pts_dev, int32_t* lm_point_dev, int32_t* n_pts_dev, snk_lmap_gather_result* out_dev)
    {
        check(snk_lmap_gather_batch_dev(h_, n_sets, &map_dev, &points_dev, frame_id_dev, local_kf_dev, par_.kf_cap, sel_dev, set_start_dev, n_set_points,
                                        set_point_dev, pts_cap, lm_pts_dev, lm_point_dev, n_pts_dev, out_dev),
              "snk_lmap_gather_batch_dev");
    }
    void Sync() { check(snk_matcher_sync(h_), "snk_matcher_sync"); }

   private:
    snk_matcher* h_ = nullptr;
    snk_lmap_params par_;
};

// LocalBundleAdjustment::MakeLocalScene, semantics "snk-scene v1" (reference Snake/Optimizer/LocalBundleAdjustment.cpp:94-346), for a
// list of keyframes: Window picks the keyframes (:124-151), Gather builds the scene (:154-346).  Scenes holds the rows as
// snk_ba_problem takes them; Problem(s, K, bf) points one at row s, to be handed to snk_ba_set_problem(s) while Scenes is alive.
// img_kf / pt_id / obs_src are kfmapinv, mpmapinv and the place of an observation in the map, for UpdateLocalScene.
class LocalSceneBuilder
{
   public:
    struct Map  // the tables of snk_scene_map and every keyframe's connections (LocalMapBuilder::Graph's layout); imu: all five or none
    {
        std::vector<uint8_t> kf_bad;
        std::vector<int32_t> kf_prev;
        std::vector<double> kf_pose;  // [n_kf][7]
        std::vector<int32_t> conn_start{0};
        std::vector<snk_covis_conn> conn_list;
        std::vector<int32_t> feat_start{0}, feat_point, feat_octave;
        std::vector<float> feat_depth, feat_uv;  // feat_uv [n_feat][2]
        std::vector<int32_t> obs_start{0}, obs;  // obs [n_obs][2]
        std::vector<uint8_t> pt_flags;
        std::vector<double> pt_pos;  // [n_points][3]
        std::vector<float> level_inv_sq_scale;
        bool imu = false;
        std::vector<double> kf_time, kf_imu_begin, kf_imu_end;
        std::vector<uint8_t> kf_preint_valid;
        std::vector<snk_ba_rpc> kf_rpc;
        snk_scene_map map() const
        {
            snk_scene_map m{};
            m.n_kf = (int32_t)kf_bad.size(), m.n_points = (int32_t)pt_flags.size(), m.n_obs = (int32_t)obs.size() / 2, m.n_feat = (int32_t)feat_point.size();
            m.n_levels = (int32_t)level_inv_sq_scale.size();
            m.kf_bad = kf_bad.data(), m.kf_prev = kf_prev.data(), m.kf_pose = kf_pose.data(), m.feat_start = feat_start.data(), m.feat_point = feat_point.data();
            m.feat_depth = feat_depth.data(), m.feat_uv = feat_uv.data(), m.feat_octave = feat_octave.data(), m.obs_start = obs_start.data();
            m.obs = reinterpret_cast<const int32_t(*)[2]>(obs.data()), m.pt_flags = pt_flags.data(), m.pt_pos = pt_pos.data();
            m.level_inv_sq_scale = level_inv_sq_scale.data();
            if (imu)
            {
                m.kf_time = kf_time.data(), m.kf_imu_begin = kf_imu_begin.data(), m.kf_imu_end = kf_imu_end.data();
                m.kf_preint_valid = kf_preint_valid.data(), m.kf_rpc = kf_rpc.data();
            }
            return m;
        }
    };
    struct Windows  // [n_q][win_cap] window keyframes (-1 past n_window) and a record per query
    {
        std::vector<int32_t> window_kf;
        std::vector<snk_scene_window_result> result;
    };
    struct Scenes  // the rows of snk_scene_out for n_q queries
    {
        int32_t win_cap = 0, pt_cap = 0, img_cap = 0, obs_cap = 0;
        std::vector<int32_t> img_kf, pt_id, obs_img, obs_pt, obs_src;
        std::vector<double> pose, pt, obs_uv, obs_depth, obs_weight;
        std::vector<uint8_t> img_const, pt_const, pt_valid;
        std::vector<snk_ba_rpc> rpc;
        std::vector<snk_scene_result> result;
        snk_scene_out out()
        {
            return snk_scene_out{win_cap,         pt_cap,          img_cap,       obs_cap,        img_kf.data(),  pose.data(),      img_const.data(),
                                 pt_id.data(),    pt.data(),       pt_const.data(), pt_valid.data(), obs_img.data(), obs_pt.data(),  obs_uv.data(),
                                 obs_depth.data(), obs_weight.data(), obs_src.data(), rpc.data(),     result.data()};
        }
        // a snk_ba_problem over row s (status SNK_SCENE_OK); K = fx fy cx cy
        snk_ba_problem Problem(size_t s, const double K[4], double bf)
        {
            if (s >= result.size() || result[s].status != SNK_SCENE_OK) throw std::invalid_argument("LocalSceneBuilder: no scene in this row");
            snk_ba_problem p{};
            p.n_img = result[s].n_img, p.n_pt = result[s].n_pt, p.n_obs = result[s].n_obs, p.n_rpc = result[s].n_rpc;
            p.pose      = reinterpret_cast<double(*)[7]>(pose.data() + s * (size_t)img_cap * 7);
            p.img_const = img_const.data() + s * (size_t)img_cap;
            p.pt        = reinterpret_cast<double(*)[3]>(pt.data() + s * (size_t)pt_cap * 3);
            p.pt_const  = pt_const.data() + s * (size_t)pt_cap;
            p.obs_img = obs_img.data() + s * (size_t)obs_cap, p.obs_pt = obs_pt.data() + s * (size_t)obs_cap;
            p.obs_uv    = reinterpret_cast<const double(*)[2]>(obs_uv.data() + s * (size_t)obs_cap * 2);
            p.obs_depth = obs_depth.data() + s * (size_t)obs_cap, p.obs_weight = obs_weight.data() + s * (size_t)obs_cap;
            for (int i = 0; i < 4; ++i) p.K[i] = K[i];
            p.bf  = bf;
            p.rpc = p.n_rpc ? rpc.data() + s * (size_t)win_cap : nullptr;
            return p;
        }
    };

    explicit LocalSceneBuilder(const snk_scene_params& params, int win_cap = 36, int device = 0) : par_(params), win_cap_(win_cap)
    {
        check(snk_matcher_create(device, nullptr, &h_), "snk_matcher_create");
    }
    ~LocalSceneBuilder() { snk_matcher_destroy(h_); }
    LocalSceneBuilder(const LocalSceneBuilder&)            = delete;
    LocalSceneBuilder& operator=(const LocalSceneBuilder&) = delete;

    Windows Window(const Map& map, const std::vector<int32_t>& q)
    {
        Windows out;
        out.window_kf.assign(q.size() * (size_t)win_cap_, -1);
        out.result.resize(q.size());
        check(snk_scene_window(h_, (int)q.size(), q.data(), (int)map.kf_bad.size(), map.kf_bad.data(), map.kf_prev.data(), map.conn_start.data(),
                               map.conn_list.data(), &par_, win_cap_, out.window_kf.data(), out.result.data()),
              "snk_scene_window");
        return out;
    }

    Scenes Gather(const Map& map, const Windows& win, int pt_cap, int img_cap, int obs_cap)
    {
        const size_t n = win.result.size(), pc = (size_t)std::max(pt_cap, 1), ic = (size_t)std::max(img_cap, 1), oc = (size_t)std::max(obs_cap, 1);
        Scenes s;
        s.win_cap = win_cap_, s.pt_cap = pt_cap, s.img_cap = img_cap, s.obs_cap = obs_cap;
        s.img_kf.assign(n * ic, -1), s.pose.assign(n * ic * 7, 0.0), s.img_const.assign(n * ic, 0);
        s.pt_id.assign(n * pc, -1), s.pt.assign(n * pc * 3, 0.0), s.pt_const.assign(n * pc, 0), s.pt_valid.assign(n * pc, 0);
        s.obs_img.assign(n * oc, -1), s.obs_pt.assign(n * oc, -1), s.obs_uv.assign(n * oc * 2, 0.0), s.obs_depth.assign(n * oc, 0.0);
        s.obs_weight.assign(n * oc, 0.0), s.obs_src.assign(n * oc * 2, -1), s.rpc.assign(n * (size_t)win_cap_, snk_ba_rpc{}), s.result.resize(n);
        const snk_scene_map m = map.map();
        const snk_scene_out o = s.out();
        check(snk_scene_gather(h_, (int)n, &m, win.window_kf.data(), win.result.data(), &par_, &o), "snk_scene_gather");
        return s;
    }

    // the device forms: every pointer is device memory, nothing is copied, the call returns before the kernel has run
    void WindowDev(int n_q, const int32_t* q_dev, int n_kf, const uint8_t* kf_bad_dev, const int32_t* kf_prev_dev, const int32_t* conn_start_dev, int n_list,
                   const snk_covis_conn* conn_list_dev, int32_t* window_kf_dev, snk_scene_window_result* out_dev)
    {
        check(snk_scene_window_batch_dev(h_, n_q, q_dev, n_kf, kf_bad_dev, kf_prev_dev, conn_start_dev, n_list, conn_list_dev, &par_, win_cap_, window_kf_dev,
                                         out_dev),
              "snk_scene_window_batch_dev");
    }
    void GatherDev(int n_q, const snk_scene_map& map_dev, const int32_t* window_kf_dev, const snk_scene_window_result* win_dev, const snk_scene_out& out_dev)
    {
        check(snk_scene_gather_batch_dev(h_, n_q, &map_dev, window_kf_dev, win_dev, &par_, &out_dev), "snk_scene_gather_batch_dev");
    }
    void Sync() { check(snk_matcher_sync(h_), "snk_matcher_sync"); }

   private:
    snk_matcher* h_ = nullptr;
    snk_scene_params par_;
    int win_cap_;
};

// Simplification::KeyFrameCullingGraph and Redundancy, semantics "snk-simp v1" (reference Snake/Optimizer/Simplification.cpp:148-358,
// :75-146; Keyframe::MatchCount and ComputeDepthRange, Snake/Map/Keyframe.cpp:68-77, :175-206) for a list of keyframes per call, with
// the reference's method names.  Map holds the tables; Map::FromObjects flattens reference-shaped Keyframe / MapPoint objects into them.
// KeyFrameCullingGraph does what the reference does around the decision: the statistics of the queries and of every live keyframe whose
// cached median is <= 0 (Keyframe.cpp:177), the fill of that cache in the Map, then the verdicts.  UpdateConnections of :207 (the
// CovisibilityGraph above), EraseKeyframe and the re-queue of the three best covisible keyframes (:50-63) stay with the caller.
class KeyframeCuller
{
   public:
    struct Map  // the tables of snk_simp_map and snk_simp_graph; times: kf_prev / kf_next / kf_time all or none
    {
        std::vector<uint8_t> kf_bad;
        std::vector<double> kf_pose;  // [n_kf][7]
        std::vector<float> kf_cull_factor;
        std::vector<double> kf_median_depth;  // the cache: KeyFrameCullingGraph fills the entries <= 0
        bool times = false;
        std::vector<int32_t> kf_prev, kf_next;
        std::vector<double> kf_time;
        std::vector<int32_t> conn_start{0};
        std::vector<snk_covis_conn> conn_list;
        std::vector<int32_t> feat_start{0}, feat_point, feat_octave;
        std::vector<float> feat_depth;
        std::vector<int32_t> obs_start{0}, obs;  // obs [n_obs][2]
        std::vector<uint8_t> pt_flags;
        std::vector<double> pt_pos;  // [n_points][3]
        snk_simp_map map() const
        {
            snk_simp_map m{};
            m.n_kf = (int32_t)kf_bad.size(), m.n_points = (int32_t)pt_flags.size(), m.n_obs = (int32_t)obs.size() / 2, m.n_feat = (int32_t)feat_point.size();
            m.kf_bad = kf_bad.data(), m.kf_pose = kf_pose.data(), m.feat_start = feat_start.data(), m.feat_point = feat_point.data();
            m.feat_depth = feat_depth.data(), m.feat_octave = feat_octave.data(), m.obs_start = obs_start.data();
            m.obs = reinterpret_cast<const int32_t(*)[2]>(obs.data()), m.pt_flags = pt_flags.data(), m.pt_pos = pt_pos.data();
            return m;
        }
        snk_simp_graph graph() const
        {
            snk_simp_graph g{};
            g.n_kf = (int32_t)kf_bad.size(), g.n_list = (int32_t)conn_list.size();
            g.kf_bad = kf_bad.data(), g.kf_pose = kf_pose.data(), g.kf_cull_factor = kf_cull_factor.data(), g.kf_median_depth = kf_median_depth.data();
            if (times) g.kf_prev = kf_prev.data(), g.kf_next = kf_next.data(), g.kf_time = kf_time.data();
            g.conn_start = conn_start.data(), g.conn_list = conn_list.data();
            return g;
        }
        // From objects shaped like the reference's.  KF: bool bad; double pose[7]; float cull_factor; double median_depth;
        // std::vector<MP*> observations (nullptr: none); std::vector<float> depth; std::vector<int> octave;
        // std::vector<std::pair<int, KF*>> connections (ascending, as GetConnections returns them); KF *previousKF, *nextKF;
        // double timeStamp; int slot.  MP: bool bad; double position[3]; std::vector<std::pair<KF*, int>> observations (GetObservationList);
        // int slot.  The slots are the positions in the two vectors.
        template <class KF, class MP>
        static Map FromObjects(const std::vector<KF*>& keyframes, const std::vector<MP*>& points, bool with_times)
        {
            Map m;
            m.times = with_times;
            for (const KF* kf : keyframes)
            {
                m.kf_bad.push_back(kf->bad ? 1 : 0);
                m.kf_pose.insert(m.kf_pose.end(), kf->pose, kf->pose + 7);
                m.kf_cull_factor.push_back(kf->cull_factor);
                m.kf_median_depth.push_back(kf->median_depth);
                if (with_times)
                {
                    m.kf_prev.push_back(kf->previousKF ? kf->previousKF->slot : -1);
                    m.kf_next.push_back(kf->nextKF ? kf->nextKF->slot : -1);
                    m.kf_time.push_back(kf->timeStamp);
                }
                for (const auto& c : kf->connections) m.conn_list.push_back(snk_covis_conn{c.first, c.second->slot});
                m.conn_start.push_back((int32_t)m.conn_list.size());
                for (size_t i = 0; i < kf->observations.size(); ++i)
                {
                    m.feat_point.push_back(kf->observations[i] ? kf->observations[i]->slot : -1);
                    m.feat_depth.push_back(kf->depth[i]);
                    m.feat_octave.push_back(kf->octave[i]);
                }
                m.feat_start.push_back((int32_t)m.feat_point.size());
            }
            for (const MP* mp : points)
            {
                m.pt_flags.push_back(mp->bad ? SNK_COVIS_PT_BAD : 0);
                m.pt_pos.insert(m.pt_pos.end(), mp->position, mp->position + 3);
                for (const auto& o : mp->observations) m.obs.push_back(o.first->slot), m.obs.push_back(o.second);
                m.obs_start.push_back((int32_t)m.obs.size() / 2);
            }
            return m;
        }
    };

    explicit KeyframeCuller(const snk_simp_params& params, const snk_simp_stats_params& stats_params, int node_cap = SNK_SIMP_MAX_NODES, int device = 0)
        : par_(params), spar_(stats_params), node_cap_(node_cap)
    {
        check(snk_matcher_create(device, nullptr, &h_), "snk_matcher_create");
    }
    ~KeyframeCuller() { snk_matcher_destroy(h_); }
    KeyframeCuller(const KeyframeCuller&)            = delete;
    KeyframeCuller& operator=(const KeyframeCuller&) = delete;

    // stage 1 for the keyframes q (min_obs: MatchCount's argument, 3 at Simplification.cpp:282)
    std::vector<snk_simp_stats_result> Stats(const Map& map, const std::vector<int32_t>& q, int min_obs = 3)
    {
        std::vector<snk_simp_stats_result> out(q.size());
        const snk_simp_map m      = map.map();
        snk_simp_stats_params par = spar_;
        par.min_obs               = min_obs;
        check(snk_simp_stats(h_, &m, &par, (int)q.size(), q.data(), out.data()), "snk_simp_stats");
        return out;
    }

    // Simplification::Redundancy (:75-146) of every q; a bad keyframe answers 0 as the reference's `return false` does
    std::vector<float> Redundancy(const Map& map, const std::vector<int32_t>& q)
    {
        std::vector<float> out;
        for (const snk_simp_stats_result& s : Stats(map, q)) out.push_back(s.redundancy);
        return out;
    }

    // Simplification::KeyFrameCullingGraph (:148-358) of every q: {cull, reason, value} and the graph's counts.  Fills map.kf_median_depth.
    std::vector<snk_simp_verdict> KeyFrameCullingGraph(Map& map, const std::vector<int32_t>& q, std::vector<snk_simp_stats_result>* stats_out = nullptr)
    {
        std::vector<int32_t> todo = q;
        for (size_t k = 0; k < map.kf_bad.size(); ++k)
            if (map.kf_median_depth[k] <= 0 && !map.kf_bad[k]) todo.push_back((int32_t)k);
        const std::vector<snk_simp_stats_result> st = Stats(map, todo);
        for (size_t i = 0; i < todo.size(); ++i)  // Keyframe.cpp:177, :199-202
        {
            const size_t k = (size_t)todo[i];
            if (map.kf_median_depth[k] <= 0 && !map.kf_bad[k] && st[i].status == SNK_SIMP_OK && st[i].n_depth > 0) map.kf_median_depth[k] = (double)st[i].median_depth;
        }
        std::vector<snk_simp_verdict> out(q.size());
        const snk_simp_graph g = map.graph();
        check(snk_simp_decide(h_, &g, &par_, node_cap_, (int)q.size(), q.data(), st.data(), out.data()), "snk_simp_decide");
        if (stats_out) stats_out->assign(st.begin(), st.begin() + (std::ptrdiff_t)q.size());
        return out;
    }

    // the device forms: every pointer is device memory, nothing is copied, the call returns before the kernel has run
    void StatsDev(const snk_simp_map& map_dev, int n_q, const int32_t* q_dev, snk_simp_stats_result* out_dev, int min_obs = 3)
    {
        snk_simp_stats_params par = spar_;
        par.min_obs               = min_obs;
        check(snk_simp_stats_batch_dev(h_, &map_dev, &par, n_q, q_dev, out_dev), "snk_simp_stats_batch_dev");
    }
    void DecideDev(const snk_simp_graph& graph_dev, int n_q, const int32_t* q_dev, const snk_simp_stats_result* stats_dev, snk_simp_verdict* out_dev)
    {
        check(snk_simp_decide_batch_dev(h_, &graph_dev, &par_, node_cap_, n_q, q_dev, stats_dev, out_dev), "snk_simp_decide_batch_dev");
    }
    void Sync() { check(snk_matcher_sync(h_), "snk_matcher_sync"); }

   private:
    snk_matcher* h_ = nullptr;
    snk_simp_params par_;
    snk_simp_stats_params spar_;
    int node_cap_;
};

// Saiga::P3PRansac as Tracking::TrackBruteForce uses it -- Snake/Tracking/TrackingCoarse.cpp:403-440, semantics "snk-p3p v1":
//   RansacParameters params; params.maxIterations = 250; params.residualThreshold = chi1 * chi1;
//   P3PRansac pnp2(params);  inliers = pnp2.solve(wps, ips, pose, inlierMatches, inlierMask);
// Vec3 / Vec2 are three / two contiguous doubles (Eigen::Vector3d / Vector2d, std::array), the pose is qx qy qz qw tx ty tz
// (world -> camera; left as it came in without a winner).  RansacParameters::threads has no meaning here; `seed` feeds the
// counter-based sampler (a call is a pure function of its arguments).
struct RansacParameters
{
    int maxIterations        = 250;
    double residualThreshold = 1e-4;
    int threads              = 1;
    uint64_t seed            = 0;
};

class P3PRansac
{
   public:
    explicit P3PRansac(const RansacParameters& params, int device = 0) : params_(params)
    {
        check(snk_matcher_create(device, nullptr, &h_), "snk_matcher_create");
    }
    ~P3PRansac() { snk_matcher_destroy(h_); }
    P3PRansac(const P3PRansac&)            = delete;
    P3PRansac& operator=(const P3PRansac&) = delete;

    template <typename Vec3, typename Vec2>
    int solve(const std::vector<Vec3>& wps, const std::vector<Vec2>& ips, double (&pose)[7], std::vector<int>& inlierMatches,
              std::vector<char>& inlierMask)
    {
        static_assert(sizeof(Vec3) == 24 && sizeof(Vec2) == 16, "world points / image points must be 3 / 2 contiguous doubles");
        if (wps.size() != ips.size()) throw std::invalid_argument("P3PRansac::solve: wps / ips sizes");
        const size_t n = wps.size();
        std::vector<uint8_t> mask(n + 1);
        std::vector<int32_t> list(n + 1);
        snk_p3p_params p{params_.maxIterations, 0, params_.residualThreshold, params_.seed};
        snk_p3p_problem q{};
        q.n              = (int32_t)n;
        q.wps            = reinterpret_cast<const double(*)[3]>(wps.data());
        q.nips           = reinterpret_cast<const double(*)[2]>(ips.data());
        q.inlier_mask    = mask.data();
        q.inlier_matches = list.data();
        std::memcpy(q.pose, pose, sizeof(q.pose));
        check(snk_p3p_ransac(h_, &p, &q, 1), "snk_p3p_ransac");
        std::memcpy(pose, q.pose, sizeof(q.pose));
        inlierMask.assign(mask.begin(), mask.begin() + (std::ptrdiff_t)n);
        inlierMatches.assign(list.begin(), list.begin() + q.inliers);
        best_iteration = q.best_iteration;
        best_solution  = q.best_solution;
        return q.inliers;
    }

    int best_iteration = -1, best_solution = -1;  // the winning hypothesis of the last solve

   private:
    RansacParameters params_;
    snk_matcher* h_ = nullptr;
};

// The `solver` member of Snake::LoopDetector as LoopDetector::solve fills and calls it -- Snake/LoopClosing/LoopDetector.cpp:152-205,
// semantics "snk-sim3 v1":
//   solver.clear();  solver.pose1 = pKF1->Pose();  solver.pose2 = pKF2->Pose();  solver.threshold = 12;  solver.camera1 = K; ...
//   solver.ips1.push_back(kp1.point);  solver.points1.push_back(solver.pose1 * pMP1->getPosition());  ...  solver.N++;
//   int its = RansacIterationsFromProbability(solver.N, 0.999, 15, 100);
//   auto [T, scale, nInliers] = solver.solve(its, compute_scale);
// SE3 is qx qy qz qw tx ty tz with points2 ~ scale * R * points1 + t (identity / 1 without a winner); pose1 / pose2 are kept for the
// caller, who multiplies the map points by them as :193-194 do (`transform`).  inlierMask is vbInliers of :200-201; `seed` feeds the
// counter-based sampler (a call is a pure function of its arguments).
inline int RansacIterationsFromProbability(int N, double probability, int minInliers, int maxIterations)
{
    return snk_ransac_iterations(N, probability, minInliers, maxIterations);
}

class RegistrationRansac
{
   public:
    using SE3  = std::array<double, 7>;
    using Vec3 = std::array<double, 3>;
    using Vec2 = std::array<double, 2>;

    explicit RegistrationRansac(int device = 0) { check(snk_matcher_create(device, nullptr, &h_), "snk_matcher_create"); }
    ~RegistrationRansac() { snk_matcher_destroy(h_); }
    RegistrationRansac(const RegistrationRansac&)            = delete;
    RegistrationRansac& operator=(const RegistrationRansac&) = delete;

    void clear()
    {
        points1.clear();
        points2.clear();
        ips1.clear();
        ips2.clear();
        inlierMask.clear();
        N = 0;
    }

    // pose * p for a pose world -> camera (the product of :193-194)
    static Vec3 transform(const SE3& pose, const Vec3& p)
    {
        const double x = pose[0], y = pose[1], z = pose[2], w = pose[3];
        const double R[9] = {1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - z * w),       2.0 * (x * z + y * w),
                             2.0 * (x * y + z * w),       1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - x * w),
                             2.0 * (x * z - y * w),       2.0 * (y * z + x * w),       1.0 - 2.0 * (x * x + y * y)};
        Vec3 o;
        for (int r = 0; r < 3; ++r) o[(size_t)r] = ((R[3 * r] * p[0] + R[3 * r + 1] * p[1]) + R[3 * r + 2] * p[2]) + pose[(size_t)(4 + r)];
        return o;
    }

    std::tuple<SE3, double, int> solve(int its, bool compute_scale)
    {
        const size_t n = points1.size();
        if (points2.size() != n || ips1.size() != n || ips2.size() != n) throw std::invalid_argument("RegistrationRansac::solve: sizes");
        std::vector<uint8_t> mask(n + 1);
        snk_sim3_params p{its, compute_scale ? 1 : 0, threshold, seed, 0.999, 15, 100};
        snk_sim3_problem q{};
        q.n           = (int32_t)n;
        q.points1     = reinterpret_cast<const double(*)[3]>(points1.data());
        q.points2     = reinterpret_cast<const double(*)[3]>(points2.data());
        q.ips1        = reinterpret_cast<const double(*)[2]>(ips1.data());
        q.ips2        = reinterpret_cast<const double(*)[2]>(ips2.data());
        q.inlier_mask = mask.data();
        q.cam         = camera1;
        q.T[3]        = 1.0;
        q.scale       = 1.0;
        check(snk_sim3_ransac(h_, &p, &q, 1), "snk_sim3_ransac");
        inlierMask.assign(mask.begin(), mask.begin() + (std::ptrdiff_t)n);
        best_iteration = q.best_iteration;
        SE3 T;
        std::memcpy(T.data(), q.T, sizeof(q.T));
        return {T, q.scale, q.inliers};
    }

    std::vector<Vec3> points1, points2;
    std::vector<Vec2> ips1, ips2;
    SE3 pose1{{0, 0, 0, 1, 0, 0, 0}}, pose2{{0, 0, 0, 1, 0, 0, 0}};
    double threshold = 12;
    int N            = 0;
    snk_camera camera1{}, camera2{};
    uint64_t seed = 0;
    std::vector<char> inlierMask;
    int best_iteration = -1;  // the winning hypothesis of the last solve

   private:
    snk_matcher* h_ = nullptr;
};

// Bag-of-words place recognition (semantics "snk-bow v1") under the reference's names:
//   ORBVocabulary vocabulary(arrays);  vocabulary.transform(descriptors, bow_vec, bow_feature_vec, 4);        // Snake/Map/Frame.cpp:38-40
//   KeyframeDatabase db(vocabulary);  db.Add(id, bow_vec);  db.DetectLoopCandidates(bv, connected, minScore, max_candidates);
//   LoopORBmatcher::MatchBoW(descriptors1, has_mp1, fv1, descriptors2, has_mp2, fv2, matches12, 50, 0.75);   // LoopDetector.cpp:225
// BowVector / FeatureVector are the ordered maps of DBoW2; a keyframe is its id.
using BowVector     = std::map<int32_t, double>;                // word -> value
using FeatureVector = std::map<uint32_t, std::vector<int32_t>>; // node -> feature indices

struct VocabularyArrays  // the flat tree of snk_bow_vocab_create (node 0 = root)
{
    std::vector<int32_t> child_start, child_count, children, word_id;
    std::vector<DescriptorORB> desc;
    std::vector<double> weight;
};

class ORBVocabulary
{
   public:
    explicit ORBVocabulary(const VocabularyArrays& a, int device = 0)
    {
        const size_t n = a.child_start.size();
        if (a.child_count.size() != n || a.word_id.size() != n || a.desc.size() != n || a.weight.size() != n)
            throw std::invalid_argument("ORBVocabulary: per-node arrays differ in length");
        check(snk_bow_vocab_create((int)n, a.child_start.data(), a.child_count.data(), a.children.data(), (int)a.children.size(),
                                   reinterpret_cast<const uint64_t(*)[4]>(a.desc.data()), a.word_id.data(), a.weight.data(), device, nullptr, &h_),
              "snk_bow_vocab_create");
    }
    ~ORBVocabulary() { snk_bow_vocab_destroy(h_); }
    ORBVocabulary(const ORBVocabulary&)            = delete;
    ORBVocabulary& operator=(const ORBVocabulary&) = delete;

    // vocabulary.transform(descriptors, bow_vec, bow_feature_vec, levelsup) -- Frame.cpp:38-40 (the thread count has no counterpart)
    void transform(const std::vector<DescriptorORB>& descriptors, BowVector& bow_vec, FeatureVector& bow_feature_vec, int levelsup) const
    {
        const size_t n = descriptors.size(), cap = n + 1;
        std::vector<int32_t> words(cap), node_start(cap + 1), features(cap), wof(cap), nof(cap);
        std::vector<uint32_t> node_id(cap);
        std::vector<double> values(cap);
        int nw = 0, nn = 0;
        check(snk_bow_transform(h_, reinterpret_cast<const uint64_t(*)[4]>(descriptors.data()), (int)n, levelsup, words.data(), values.data(), &nw,
                                node_id.data(), node_start.data(), features.data(), &nn, wof.data(), nof.data()),
              "snk_bow_transform");
        bow_vec.clear();
        bow_feature_vec.clear();
        for (int i = 0; i < nw; ++i) bow_vec.emplace_hint(bow_vec.end(), words[(size_t)i], values[(size_t)i]);
        for (int i = 0; i < nn; ++i)
            bow_feature_vec.emplace_hint(bow_feature_vec.end(), node_id[(size_t)i],
                                         std::vector<int32_t>(features.begin() + node_start[(size_t)i], features.begin() + node_start[(size_t)i + 1]));
    }
    // vocabulary.score(a, b) -- LoopDetector.cpp:73
    double score(const BowVector& a, const BowVector& b) const
    {
        std::vector<int32_t> wa, wb;
        std::vector<double> va, vb;
        flatten(a, wa, va);
        flatten(b, wb, vb);
        double s = 0.0;
        check(snk_bow_score(h_, wa.data(), va.data(), (int)wa.size(), wb.data(), vb.data(), (int)wb.size(), &s), "snk_bow_score");
        return s;
    }
    int size() const
    {
        int n = 0;
        check(snk_bow_vocab_size(h_, &n, nullptr, nullptr), "snk_bow_vocab_size");
        return n;
    }
    static void flatten(const BowVector& v, std::vector<int32_t>& words, std::vector<double>& values)
    {
        words.clear();
        values.clear();
        for (const auto& e : v)
        {
            words.push_back(e.first);
            values.push_back(e.second);
        }
    }
    snk_bow_vocab* handle() const { return h_; }

   private:
    snk_bow_vocab* h_ = nullptr;
};

// Snake::KeyframeDatabase -- Snake/LoopClosing/KeyframeDatabase.cpp:20-168
class KeyframeDatabase
{
   public:
    explicit KeyframeDatabase(ORBVocabulary& vocabulary, int maxKeyframes = 10000, int maxWords = SNK_BOW_MAX_FEATURES)
    {
        check(snk_bow_db_create(vocabulary.handle(), maxKeyframes, maxWords, &h_), "snk_bow_db_create");
    }
    ~KeyframeDatabase() { snk_bow_db_destroy(h_); }
    KeyframeDatabase(const KeyframeDatabase&)            = delete;
    KeyframeDatabase& operator=(const KeyframeDatabase&) = delete;

    void Add(int kf_id, const BowVector& bv)
    {
        std::vector<int32_t> w;
        std::vector<double> v;
        ORBVocabulary::flatten(bv, w, v);
        check(snk_bow_db_add(h_, kf_id, w.data(), v.data(), (int)w.size()), "snk_bow_db_add");
    }
    void Remove(int kf_id) { check(snk_bow_db_remove(h_, kf_id), "snk_bow_db_remove"); }
    // :58-80: (keyframe id, score), best first
    std::vector<std::pair<int, float>> DetectLoopCandidates(const BowVector& bv, const std::vector<int>& connected_keyframes, float minScore,
                                                            int max_candidates)
    {
        return query(bv, connected_keyframes, minScore, max_candidates);
    }
    // :83-98: the reference passes 0 as the score floor whatever minScore is (:89)
    std::vector<std::pair<int, float>> DetectRelocalizationCandidates(const BowVector& bv, float /*minScore*/, int max_candidates)
    {
        return query(bv, {}, 0.0f, max_candidates);
    }

   private:
    std::vector<std::pair<int, float>> query(const BowVector& bv, const std::vector<int>& exclude, float min_score, int max_candidates)
    {
        std::vector<int32_t> w, ids((size_t)max_candidates + 1), ex(exclude.begin(), exclude.end());
        std::vector<double> v, scores((size_t)max_candidates + 1);
        ORBVocabulary::flatten(bv, w, v);
        int n = 0;
        check(snk_bow_db_query(h_, w.data(), v.data(), (int)w.size(), ex.data(), (int)ex.size(), 0.8f, 0.75f, min_score, max_candidates, ids.data(),
                               scores.data(), nullptr, &n),
              "snk_bow_db_query");
        std::vector<std::pair<int, float>> out;
        for (int i = 0; i < n; ++i) out.emplace_back(ids[(size_t)i], (float)scores[(size_t)i]);
        return out;
    }
    snk_bow_db* h_ = nullptr;
};

// Snake::LoopORBmatcher -- Snake/LoopClosing/LoopORBMatcher.cpp:121-215
class LoopORBmatcher
{
   public:
    explicit LoopORBmatcher(int device = 0) { check(snk_matcher_create(device, nullptr, &h_), "snk_matcher_create"); }
    ~LoopORBmatcher() { snk_matcher_destroy(h_); }
    LoopORBmatcher(const LoopORBmatcher&)            = delete;
    LoopORBmatcher& operator=(const LoopORBmatcher&) = delete;

    // MatchBoW(pKF1, pKF2, vpMatches12, threshold, ratio): matches12[i] = the feature of keyframe 2 whose map point vpMatches12[i] holds, or -1
    int MatchBoW(const std::vector<DescriptorORB>& descriptors1, const std::vector<uint8_t>& has_mp1, const FeatureVector& fv1,
                 const std::vector<DescriptorORB>& descriptors2, const std::vector<uint8_t>& has_mp2, const FeatureVector& fv2,
                 std::vector<int32_t>& matches12, int threshold, float ratio)
    {
        if (has_mp1.size() != descriptors1.size() || has_mp2.size() != descriptors2.size()) throw std::invalid_argument("MatchBoW: sizes");
        const auto b1 = MappingORBMatcher::BowFeatureVector::from(fv1), b2 = MappingORBMatcher::BowFeatureVector::from(fv2);
        const snk_bow_features f1 = b1.view(), f2 = b2.view();
        std::vector<int32_t> m(descriptors1.size() + 1, -1);
        int n = 0;
        check(snk_match_loop_bow(h_, reinterpret_cast<const uint64_t(*)[4]>(descriptors1.data()), has_mp1.data(), (int)descriptors1.size(), &f1,
                                 reinterpret_cast<const uint64_t(*)[4]>(descriptors2.data()), has_mp2.data(), (int)descriptors2.size(), &f2, threshold,
                                 ratio, m.data(), &n),
              "snk_match_loop_bow");
        matches12.assign(m.begin(), m.begin() + (std::ptrdiff_t)descriptors1.size());
        return n;
    }

   private:
    snk_matcher* h_ = nullptr;
};


// The pose graph of LoopClosing::ConstructPGO and its solvers (reference Snake/LoopClosing/LoopClosingPGO.cpp:16-118, :120-264; semantics
// "snk-pgo v1"), used as OptimizeEssentialGraph does:
//   PoseGraph pg(poses, constant, fixScale);  pg.AddVertexEdge(i, j, weight); ...  pg.sortEdges();  pg.SetPose(source, T_w_correctSource);
//   PGORec rec (or PGOSim3Rec);  rec.optimizationOptions = ...;  rec.create(pg);  auto result = rec.initAndSolve();   // :134-146
//   rec.poses() ...;  TransformMapPoints(rec, ref, positions, normals, referenceDepth);                               // :231-260
// A Sim3 is qx qy qz qw tx ty tz s.  AddVertexEdge measures T_i_j at the poses the graph was built with (:105); SetPose (:114) moves a
// vertex afterwards without touching those measurements.
struct PoseGraph
{
    using Sim3 = std::array<double, 8>;
    struct Edge
    {
        int from, to;
        double weight;
    };
    PoseGraph() = default;
    PoseGraph(std::vector<Sim3> p, std::vector<uint8_t> c, bool fix) : posesMeasure(p), poses(std::move(p)), constant(std::move(c)), fixScale(fix) {}
    void AddVertexEdge(int i, int j, double weight = 1.0) { edges.push_back(i < j ? Edge{i, j, weight} : Edge{j, i, weight}); }
    void sortEdges()  // by (from, to); of several edges between one pair the first one added stays
    {
        std::stable_sort(edges.begin(), edges.end(), [](const Edge& a, const Edge& b) { return a.from != b.from ? a.from < b.from : a.to < b.to; });
        edges.erase(std::unique(edges.begin(), edges.end(), [](const Edge& a, const Edge& b) { return a.from == b.from && a.to == b.to; }), edges.end());
    }
    void SetPose(int i, const Sim3& T) { poses.at((size_t)i) = T; }
    std::vector<Sim3> posesMeasure, poses;
    std::vector<uint8_t> constant;
    std::vector<Edge> edges;
    bool fixScale = true;
};

class PGOBase
{
   public:
    PGOBase(const PGOBase&)            = delete;
    PGOBase& operator=(const PGOBase&) = delete;
    ~PGOBase() { snk_pgo_destroy(h_); }

    snk_pgo_options optimizationOptions{50, 10000, 1e-20, 1e-10, 1e-4};  // maxIterations, minChi2Delta: LoopClosingPGO.cpp:125-126

    void create(const PoseGraph& pg)
    {
        if (pg.fixScale != fix_) throw std::invalid_argument("PGORec solves fixScale graphs, PGOSim3Rec the others");
        if (pg.posesMeasure.size() != pg.poses.size() || pg.constant.size() != pg.poses.size()) throw std::invalid_argument("PoseGraph: array sizes");
        if (h_) snk_pgo_destroy(h_);
        h_ = nullptr;
        check(snk_pgo_create(&optimizationOptions, device_, nullptr, &h_), "snk_pgo_create");
        std::vector<int32_t> e;
        std::vector<double> w;
        for (const auto& x : pg.edges) e.push_back(x.from), e.push_back(x.to), w.push_back(x.weight);
        n_ = (int)pg.poses.size();
        check(snk_pgo_set_graph(h_, n_, reinterpret_cast<const double(*)[8]>(pg.posesMeasure.data()), reinterpret_cast<const double(*)[8]>(pg.poses.data()),
                                pg.constant.data(), (int)pg.edges.size(), reinterpret_cast<const int32_t(*)[2]>(e.data()), w.data(), nullptr, fix_ ? 1 : 0),
              "snk_pgo_set_graph");
    }
    snk_pgo_result initAndSolve()
    {
        snk_pgo_result r{};
        check(snk_pgo_solve(handle(), &r), "snk_pgo_solve");
        return r;
    }
    std::vector<PoseGraph::Sim3> poses()
    {
        std::vector<PoseGraph::Sim3> out((size_t)n_);
        check(snk_pgo_get_poses(handle(), reinterpret_cast<double(*)[8]>(out.data())), "snk_pgo_get_poses");
        return out;
    }
    snk_pgo* handle()
    {
        if (!h_) throw std::logic_error("PGO: create(pg) first");
        return h_;
    }

   protected:
    PGOBase(bool fix, int device) : fix_(fix), device_(device) {}

   private:
    bool fix_;
    int device_;
    int n_      = 0;
    snk_pgo* h_ = nullptr;
};
class PGORec : public PGOBase
{
   public:
    explicit PGORec(int device = 0) : PGOBase(true, device) {}
};
class PGOSim3Rec : public PGOBase
{
   public:
    explicit PGOSim3Rec(int device = 0) : PGOBase(false, device) {}
};

// The map-point pass of OptimizeEssentialGraph (:231-247, MapPoint::Transform at :256-260): normals / referenceDepth may be empty.
inline void TransformMapPoints(PGOBase& rec, const std::vector<int32_t>& referenceVertex, std::vector<std::array<double, 3>>& positions,
                               std::vector<std::array<double, 3>>& normals, std::vector<double>& referenceDepth)
{
    const size_t n = referenceVertex.size();
    if (positions.size() != n || (!normals.empty() && normals.size() != n) || (!referenceDepth.empty() && referenceDepth.size() != n))
        throw std::invalid_argument("TransformMapPoints: sizes");
    check(snk_pgo_transform_points(rec.handle(), (int)n, referenceVertex.data(), reinterpret_cast<double(*)[3]>(positions.data()),
                                   normals.empty() ? nullptr : reinterpret_cast<double(*)[3]>(normals.data()),
                                   referenceDepth.empty() ? nullptr : referenceDepth.data()),
          "snk_pgo_transform_points");
}


// Snake::PoseRefinement (reference Snake/Tracking/PoseRefinement.h:22-99): the robust pose-only
// optimisation after every matcher call.  The caller gathers wps / obs / idx exactly as refinePose
// (:35-60) and RefinePoseWithMatches (PoseRefinement.cpp:37-57) do, then writes outlier[i] to
// frame.mvbOutlier[idx[i]] and the pose to frame.setPose().
class PoseRefinement
{
   public:
    explicit PoseRefinement(double errorFactor = 1.0, int device = 0)
    {
        check(snk_matcher_create(device, nullptr, &h_), "snk_matcher_create");
        options.th_mono          = 2.1 * errorFactor;  // reprojectionErrorThresholdMono, SnakeGlobal.h:145
        options.th_stereo        = 2.3 * errorFactor;  // reprojectionErrorThresholdStereo, SnakeGlobal.h:146
        options.outer_iterations = 4;
        options.inner_iterations = 10;
        options.robust_rounds    = 3;
        options.pad              = 0;
        options.lambda           = 1e-4;
    }
    ~PoseRefinement() { snk_matcher_destroy(h_); }
    PoseRefinement(const PoseRefinement&)            = delete;
    PoseRefinement& operator=(const PoseRefinement&) = delete;

    // rpo.optimizePoseRobust(wps, obs, outlier, pose, cam); with prediction weights > 0 the
    // rpo_smooth variant (PoseRefinement.h:68-73).  Returns the inlier count.
    int optimizePoseRobust(const std::vector<std::array<double, 3>>& wps, const std::vector<snk_pose_obs>& obs,
                           std::vector<uint8_t>& outlier, double pose[7], const snk_camera& cam,
                           const double* prediction = nullptr, double weight_rotation = 0, double weight_translation = 0)
    {
        outlier.assign(obs.size() + 1, 0);
        snk_pose_problem P{};
        P.n       = (int)obs.size();
        P.wps     = reinterpret_cast<const double(*)[3]>(wps.data());
        P.obs     = obs.data();
        P.outlier = outlier.data();
        for (int i = 0; i < 7; ++i) P.pose[i] = pose[i], P.prediction[i] = prediction ? prediction[i] : pose[i];
        P.w_rot   = prediction ? weight_rotation : 0;
        P.w_trans = prediction ? weight_translation : 0;
        check(snk_pose_refine(h_, &cam, &options, &P, 1), "snk_pose_refine");
        for (int i = 0; i < 7; ++i) pose[i] = P.pose[i];
        outlier.resize(obs.size());
        return P.inliers;
    }
    // a whole batch of frames in one launch
    void optimizeBatch(std::vector<snk_pose_problem>& problems, const snk_camera& cam)
    {
        check(snk_pose_refine(h_, &cam, &options, problems.data(), (int)problems.size()), "snk_pose_refine");
    }

    snk_pose_options options{};

   private:
    snk_matcher* h_ = nullptr;
};

// The part of Saiga::Scene that MakeLocalScene fills (LocalBundleAdjustment.cpp:187-293), flattened.
struct Scene
{
    std::vector<std::array<double, 7>> poses;  // images[i].se3: qx qy qz qw tx ty tz
    std::vector<uint8_t> image_constant;
    std::vector<std::array<double, 3>> points;  // worldPoints[j].p
    std::vector<uint8_t> point_constant;
    std::vector<int32_t> obs_image, obs_point;      // StereoImagePoint owner image, .wp
    std::vector<std::array<double, 2>> obs_pixel;   // .point
    std::vector<double> obs_depth, obs_weight;      // .depth (> 0 => stereo), .weight
    std::vector<uint8_t> obs_outlier;               // .outlier
    double K[4] = {1, 1, 0, 0};                     // intrinsics[0]
    double bf   = 0;
    std::vector<snk_ba_rpc> rel_pose_constraints;   // scene.rel_pose_constraints (IMU), LocalBundleAdjustment.cpp:294-346
};

struct OptimizationResults
{
    double cost_initial = 0, cost_final = 0;
};

// Saiga::BARecRel as Snake drives it — Snake/Optimizer/LocalBundleAdjustment.cpp:357-365,403-407
class BARec
{
   public:
    snk_ba_options optimizationOptions{3, 30, 1e-10, 2.1, 2.3, 0.0};  // LocalBundleAdjustment.cpp:47-64
    // BAOptions::buildExplizitSchur: set by the local BA (LocalBundleAdjustment.cpp:59), left unset by the global BA
    // (GlobalBundleAdjustment.cpp:32-43) -- false selects the implicit Schur form (snk_ba_set_explicit_schur); read by create()
    bool buildExplizitSchur = true;

    explicit BARec(int device = 0) : device_(device) {}
    ~BARec() { snk_ba_destroy(h_); }
    BARec(const BARec&)            = delete;
    BARec& operator=(const BARec&) = delete;

    void create(Scene& scene)
    {
        scene_ = &scene;
        // the handle (device buffers, pinned staging) survives from scene to scene; only changed options need a new one
        if (h_ && std::memcmp(&created_with_, &optimizationOptions, sizeof(snk_ba_options)) != 0)
        {
            snk_ba_destroy(h_);
            h_ = nullptr;
        }
        if (!h_)
        {
            check(snk_ba_create(&optimizationOptions, device_, nullptr, &h_), "snk_ba_create");
            created_with_ = optimizationOptions;
        }
        snk_ba_problem p{};
        p.n_img      = (int)scene.poses.size();
        p.n_pt       = (int)scene.points.size();
        p.n_obs      = (int)scene.obs_image.size();
        p.pose       = reinterpret_cast<double(*)[7]>(scene.poses.data());
        p.pt         = reinterpret_cast<double(*)[3]>(scene.points.data());
        // BAPointOnly holds every image, BAPoseOnly every point (GlobalBundleAdjustment.cpp:103-122, 306-316)
        all_const_.assign(std::max(scene.poses.size(), scene.points.size()) + 1, 1);
        p.img_const  = hold_images_ ? all_const_.data() : scene.image_constant.data();
        p.pt_const   = hold_points_ ? all_const_.data() : scene.point_constant.data();
        p.obs_img    = scene.obs_image.data();
        p.obs_pt     = scene.obs_point.data();
        p.obs_uv     = reinterpret_cast<const double(*)[2]>(scene.obs_pixel.data());
        p.obs_depth  = scene.obs_depth.data();
        p.obs_weight = scene.obs_weight.data();
        for (int k = 0; k < 4; ++k) p.K[k] = scene.K[k];
        p.bf    = scene.bf;
        p.n_rpc = (int)scene.rel_pose_constraints.size();
        p.rpc   = scene.rel_pose_constraints.data();
        check(snk_ba_set_explicit_schur(h_, buildExplizitSchur ? 1 : 0), "snk_ba_set_explicit_schur");
        check(snk_ba_set_problem(h_, &p), "snk_ba_set_problem");
    }
    // The hand-over from DEVICE rows (snk_ba_set_problems_dev): out_dev is what LocalSceneBuilder's device form filled, a host struct of
    // device pointers; problem s is row s, a row whose status is not SNK_SCENE_OK an empty problem.  The rows must be complete on the
    // handle's stream (the default one here) or their producer synchronised.  No Scene stands behind these problems: solveAll() and
    // handle() (snk_ba_get_state, snk_ba_residuals, snk_ba_solve_local_scene per problem) read the results.
    void createDev(int n_q, const snk_scene_out& out_dev, const double K[4], double bf)
    {
        scene_ = nullptr;
        count_ = 0;
        if (h_ && std::memcmp(&created_with_, &optimizationOptions, sizeof(snk_ba_options)) != 0)
        {
            snk_ba_destroy(h_);
            h_ = nullptr;
        }
        if (!h_)
        {
            check(snk_ba_create(&optimizationOptions, device_, nullptr, &h_), "snk_ba_create");
            created_with_ = optimizationOptions;
        }
        check(snk_ba_set_explicit_schur(h_, buildExplizitSchur ? 1 : 0), "snk_ba_set_explicit_schur");
        check(snk_ba_set_problems_dev(h_, n_q, &out_dev, K, bf), "snk_ba_set_problems_dev");
        count_ = n_q;
    }
    // initAndSolve() of every problem createDev loaded
    std::vector<OptimizationResults> solveAll()
    {
        std::vector<double> ci((size_t)count_ + 1), cf((size_t)count_ + 1);
        check(snk_ba_solve(h_, optimizationOptions.max_iterations, ci.data(), cf.data()), "snk_ba_solve");
        std::vector<OptimizationResults> r((size_t)count_);
        for (int b = 0; b < count_; ++b) r[(size_t)b].cost_initial = ci[(size_t)b], r[(size_t)b].cost_final = cf[(size_t)b];
        return r;
    }
    snk_ba* handle() const { return h_; }
    OptimizationResults initAndSolve() { return solve(); }
    OptimizationResults solve()
    {
        if (!scene_->obs_outlier.empty()) check(snk_ba_set_outliers(h_, 0, scene_->obs_outlier.data()), "snk_ba_set_outliers");
        OptimizationResults r;
        check(snk_ba_solve(h_, optimizationOptions.max_iterations, &r.cost_initial, &r.cost_final), "snk_ba_solve");
        // the reference mutates the scene in place
        check(snk_ba_get_state(h_, 0, reinterpret_cast<double(*)[7]>(scene_->poses.data()),
                               reinterpret_cast<double(*)[3]>(scene_->points.data()), nullptr),
              "snk_ba_get_state");
        return r;
    }
    // LocalBundleAdjustment::SolveLocalScene after create() in one library call (LocalBundleAdjustment.cpp:357-410): initAndSolve,
    // the chi-square pass on the device, one more iteration when anything was marked.  The scene's poses, points and
    // obs_outlier are updated; *outlierPoints = how many observations the pass marked; returns the FIRST solve's costs (:412).
    OptimizationResults solveLocalScene(double chi2Mono, double chi2Stereo, int* outlierPoints)
    {
        if (scene_->obs_outlier.size() != scene_->obs_image.size()) scene_->obs_outlier.assign(scene_->obs_image.size(), 0);
        bool any = false;
        for (uint8_t f : scene_->obs_outlier) any |= f != 0;
        check(snk_ba_set_outliers(h_, 0, any ? scene_->obs_outlier.data() : nullptr), "snk_ba_set_outliers");  // NULL: a device memset
        OptimizationResults r;
        int marked = 0;
        scene_->obs_outlier.push_back(0);  // never hand out a null pointer for an empty scene
        check(snk_ba_solve_local_scene(h_, 0, chi2Mono, chi2Stereo, 1, scene_->obs_outlier.data(), &marked, &r.cost_initial, &r.cost_final,
                                       reinterpret_cast<double(*)[7]>(scene_->poses.data()),
                                       reinterpret_cast<double(*)[3]>(scene_->points.data())),
              "snk_ba_solve_local_scene");
        scene_->obs_outlier.pop_back();
        if (outlierPoints) *outlierPoints = marked;
        return r;
    }
    // squared norms of Scene::residual3 / residual2 for every observation
    std::vector<double> residualsSquared()
    {
        std::vector<double> chi2(scene_->obs_image.size() + 1);
        check(snk_ba_residuals(h_, 0, chi2.data()), "snk_ba_residuals");
        chi2.resize(scene_->obs_image.size());
        return chi2;
    }

   protected:
    bool hold_images_ = false, hold_points_ = false;

   private:
    int device_;
    snk_ba* h_    = nullptr;
    Scene* scene_ = nullptr;
    int count_    = 0;  // problems createDev loaded
    snk_ba_options created_with_{};
    std::vector<uint8_t> all_const_;
};

// Saiga::BAPointOnly as GlobalBundleAdjustment::PointBA uses it (GlobalBundleAdjustment.cpp:103-122): create(scene),
// initAndSolve() -- world points optimised, every camera held.  [DEFINED]: the BARec iteration with every image constant.
class BAPointOnly : public BARec
{
   public:
    explicit BAPointOnly(int device = 0) : BARec(device)
    {
        optimizationOptions = {4, 40, 1e-10, 2.1, 2.3, 0.0};  // GlobalBundleAdjustment.cpp:32-43
        hold_images_        = true;
    }
};

// Saiga::BAPoseOnly as RealignIntermiediateFrames uses it (GlobalBundleAdjustment.cpp:306-316): camera poses optimised, every
// world point held.  [DEFINED]: the BARec iteration with every point constant.
class BAPoseOnly : public BARec
{
   public:
    explicit BAPoseOnly(int device = 0) : BARec(device)
    {
        optimizationOptions = {4, 40, 1e-10, 2.1, 2.3, 0.0};
        hold_points_        = true;
    }
};

// ------------------------------------------------------------------------------------------------
// The `.features` cache either side of the extractor — reference
// Snake/Preprocess/FeatureDetector.cpp:94-111 (read) and :134-139 / :166-171 (write):
//   BinaryFile << std::vector<Saiga::KeyPoint<double>> << std::vector<DescriptorORB>
// Saiga::BinaryFile (absent submodule) streams a vector as its element count followed by the raw
// elements.  ASSUMED layout (unverified against a file written by a real Snake-SLAM build): count as
// 64-bit little-endian size_t; KeyPoint<double> = {Vec2d point; double size, angle, response;
// int octave;} padded to 48 bytes; DescriptorORB = 32 bytes.
// ------------------------------------------------------------------------------------------------
struct KeyPointD
{
    double x, y;
    double size, angle, response;
    int32_t octave;
    int32_t pad;
};
static_assert(sizeof(KeyPointD) == 48, "KeyPoint<double> layout");

inline void WriteFeatures(const std::string& file, const std::vector<KeyPointD>& keypoints,
                          const std::vector<DescriptorORB>& descriptors)
{
    // The layout is an unverified assumption (Saiga::BinaryFile is absent): a cache written here may be silently misread by a
    // real Snake-SLAM build.  Refuse unless the caller acknowledges that (or has pinned the layout with tools/check_features_dir.py).
    const char* ack = std::getenv("SNK_FEATURES_LAYOUT_ACK");
    if (!ack || std::string(ack) != "1")
        throw std::runtime_error("WriteFeatures: the .features layout is an unverified assumption; set SNK_FEATURES_LAYOUT_ACK=1 to write it anyway");
    FILE* f = std::fopen(file.c_str(), "wb");
    if (!f) throw std::runtime_error("cannot open " + file);
    const uint64_t nk = keypoints.size(), nd = descriptors.size();
    bool ok = std::fwrite(&nk, 8, 1, f) == 1 && (nk == 0 || std::fwrite(keypoints.data(), sizeof(KeyPointD), nk, f) == nk) &&
              std::fwrite(&nd, 8, 1, f) == 1 && (nd == 0 || std::fwrite(descriptors.data(), 32, nd, f) == nd);
    ok = (std::fclose(f) == 0) && ok;
    if (!ok) throw std::runtime_error("short write to " + file);
}

inline void ReadFeatures(const std::string& file, std::vector<KeyPointD>& keypoints, std::vector<DescriptorORB>& descriptors)
{
    FILE* f = std::fopen(file.c_str(), "rb");
    if (!f) throw std::runtime_error("cannot open " + file);
    auto fail = [&](const char* what) {
        std::fclose(f);
        throw std::runtime_error(std::string(what) + " in " + file);
    };
    uint64_t nk = 0, nd = 0;
    if (std::fread(&nk, 8, 1, f) != 1 || nk > (1u << 24)) fail("bad keypoint count");
    keypoints.resize(nk);
    if (nk && std::fread(keypoints.data(), sizeof(KeyPointD), nk, f) != nk) fail("truncated keypoints");
    if (std::fread(&nd, 8, 1, f) != 1 || nd > (1u << 24)) fail("bad descriptor count");
    descriptors.resize(nd);
    if (nd && std::fread(descriptors.data(), 32, nd, f) != nd) fail("truncated descriptors");
    std::fclose(f);
}

// A file of unknown provenance (a real Snake-SLAM build: saiga's BinaryFile layout is not known here): tries the plausible
// layouts -- 64 / 32-bit counts; KeyPoint<double> of 48 bytes, packed 44, KeyPoint<float> of 24 -- and keeps the first one
// that accounts for every byte of the file (same probing as snake_slam_amd/features_io.py::probe_layout).  Returns the layout
// as "count bytes / keypoint bytes", e.g. "8/48".
inline std::string ReadFeaturesAny(const std::string& file, std::vector<KeyPointD>& keypoints, std::vector<DescriptorORB>& descriptors)
{
    FILE* f = std::fopen(file.c_str(), "rb");
    if (!f) throw std::runtime_error("cannot open " + file);
    std::vector<unsigned char> buf;
    unsigned char tmp[65536];
    size_t got;
    while ((got = std::fread(tmp, 1, sizeof(tmp), f)) > 0) buf.insert(buf.end(), tmp, tmp + got);
    std::fclose(f);
    auto rd = [&](size_t off, int bytes) {
        uint64_t v = 0;
        for (int i = 0; i < bytes; ++i) v |= (uint64_t)buf[off + (size_t)i] << (8 * i);
        return v;
    };
    for (int cw : {8, 4})
        for (int ks : {48, 44, 24})
        {
            if (buf.size() < 2 * (size_t)cw) continue;
            const uint64_t nk = rd(0, cw);
            const size_t off  = (size_t)cw + (size_t)nk * (size_t)ks;
            if (nk > (1u << 24) || off + (size_t)cw > buf.size()) continue;
            const uint64_t nd = rd(off, cw);
            if (nd != nk || off + (size_t)cw + (size_t)nd * 32 != buf.size()) continue;
            keypoints.resize(nk);
            descriptors.resize(nd);
            for (uint64_t i = 0; i < nk; ++i)
            {
                const unsigned char* p = buf.data() + cw + i * (size_t)ks;
                KeyPointD k{};
                if (ks == 24)
                {
                    float v[5];
                    std::memcpy(v, p, 20);
                    std::memcpy(&k.octave, p + 20, 4);
                    k.x = v[0], k.y = v[1], k.size = v[2], k.angle = v[3], k.response = v[4];
                }
                else
                {
                    double v[5];
                    std::memcpy(v, p, 40);
                    std::memcpy(&k.octave, p + 40, 4);
                    k.x = v[0], k.y = v[1], k.size = v[2], k.angle = v[3], k.response = v[4];
                }
                keypoints[i] = k;
            }
            if (nd) std::memcpy(descriptors.data(), buf.data() + off + cw, (size_t)nd * 32);
            return std::to_string(cw) + "/" + std::to_string(ks);
        }
    throw std::runtime_error("no known layout accounts for the size of " + file);
}

// frame.keypoints.emplace_back(kp.cast<double>()) — FeatureDetector.cpp:128-131
inline KeyPointD cast_double(const snk_keypoint& k)
{
    return KeyPointD{(double)k.x, (double)k.y, (double)k.size, (double)k.angle, (double)k.response, k.octave, 0};
}
// ------------------------------------------------------------------------------------------------
// One Snake-SLAM process per GPU (BASELINE config 5): gather every rank's results with RCCL over xGMI, no MPI / torch in the process.
// A rank's block is what System::writeFrameTrajectory writes for its sequence (Snake/System/System.cpp:546-563): one
// {timestamp, tx, ty, tz, qx, qy, qz, qw} row per frame with a valid pose.
// ------------------------------------------------------------------------------------------------
struct TumPose
{
    double t, tx, ty, tz, qx, qy, qz, qw;
};

class Dist
{
   public:
    // rendezvous through a file all ranks see (snk_dist_init_file): a fresh path per job
    Dist(const std::string& rendezvous_file, int rank, int world, int device, double timeout_s = 60.0)
    {
        check(snk_dist_init_file(rendezvous_file.c_str(), rank, world, device, timeout_s, &h_), "snk_dist_init_file");
        rank_ = rank;
        world_ = world;
        if (rank == 0) file_ = rendezvous_file;
    }
    // the 128-byte id was handed around by the launcher
    Dist(const uint8_t id[SNK_DIST_ID_BYTES], int rank, int world, int device)
    {
        check(snk_dist_init(id, rank, world, device, &h_), "snk_dist_init");
        rank_ = rank;
        world_ = world;
    }
    ~Dist()
    {
        snk_dist_destroy(h_);
        if (!file_.empty()) std::remove(file_.c_str());
    }
    Dist(const Dist&)            = delete;
    Dist& operator=(const Dist&) = delete;
    int rank() const { return rank_; }
    snk_dist* handle() const { return h_; }  // for snk_dist_rank (what the communicator itself reports)
    int world() const { return world_; }

    // all ranks' trajectories on every rank: result[r] = rank r's rows.  Two collectives: the longest trajectory (blocks are padded to
    // it), then ONE all-gather of {n, rows} blocks -- the exchange SURVEY.md section 8e describes (~236 KB per rank for MH_01).
    std::vector<std::vector<TumPose>> GatherTrajectories(const std::vector<TumPose>& mine)
    {
        int64_t longest = 0;
        check(snk_dist_max_i64(h_, (int64_t)mine.size(), &longest), "snk_dist_max_i64");
        const size_t block = 8 + (size_t)longest * sizeof(TumPose);  // {int64 n, rows}
        std::vector<uint8_t> send(block, 0), recv(block * (size_t)world_);
        const int64_t n = (int64_t)mine.size();
        std::memcpy(send.data(), &n, 8);
        if (n) std::memcpy(send.data() + 8, mine.data(), (size_t)n * sizeof(TumPose));
        check(snk_dist_all_gather(h_, send.data(), block, recv.data()), "snk_dist_all_gather");
        std::vector<std::vector<TumPose>> all((size_t)world_);
        for (int r = 0; r < world_; ++r)
        {
            int64_t nr = 0;
            std::memcpy(&nr, recv.data() + (size_t)r * block, 8);
            all[(size_t)r].resize((size_t)nr);
            if (nr) std::memcpy(all[(size_t)r].data(), recv.data() + (size_t)r * block + 8, (size_t)nr * sizeof(TumPose));
        }
        return all;
    }
    // any fixed-size block per rank (counters: frames, frames/s, matches, BA costs)
    template <typename T>
    std::vector<T> GatherBlocks(const T& mine)
    {
        static_assert(std::is_trivially_copyable<T>::value, "plain data only");
        std::vector<T> all((size_t)world_);
        check(snk_dist_all_gather(h_, &mine, sizeof(T), all.data()), "snk_dist_all_gather");
        return all;
    }

   private:
    snk_dist* h_ = nullptr;
    int rank_ = 0, world_ = 1;
    std::string file_;
};
}  // namespace snake_hip
