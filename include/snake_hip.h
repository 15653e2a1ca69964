/*
 * snake_hip.h — C ABI of the MI355X (gfx950) implementation of Snake-SLAM's
 * per-frame feature pipeline and local bundle adjustment.
 *
 * Every entry point replaces one seam of the reference (darglein/Snake-SLAM);
 * the seam is cited as `path:line` relative to the reference checkout.  The
 * reference has no FFI layer: its seams are C++ member calls into the (absent)
 * saiga submodule, so a C++ adaptor on the Snake side converts std::vector /
 * Eigen to the plain pointers used here (see INTEGRATION.md and
 * snake_slam_amd/cpp/snake_hip.hpp).
 *
 * Conventions
 *  - all functions return an snk_status (0 = ok); nothing aborts or throws;
 *  - "host" entry points take host pointers, are synchronous, and copy through
 *    buffers owned by the handle (the reference's call shape);
 *  - "_dev" entry points take device pointers, enqueue on the handle's stream and
 *    return without synchronising (batched throughput path; inputs resident in HBM);
 *  - a handle is used by one thread at a time; different handles are independent
 *    (reference threading: FeatureDetection || Preprocess || Tracking || LBA);
 *  - a descriptor is 256 bits = 4 x uint64_t, little-endian bit order: bit b of the
 *    descriptor is bit (b & 63) of word (b >> 6).
 */
#ifndef SNAKE_HIP_H
#define SNAKE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SNK_API __attribute__((visibility("default")))

typedef enum snk_status
{
    SNK_OK                = 0,
    SNK_ERR_INVALID_ARG   = 1,
    SNK_ERR_NO_DEVICE     = 2, /* no HIP device / HIP runtime failure at create */
    SNK_ERR_HIP           = 3, /* a HIP call failed; see snk_last_error() */
    SNK_ERR_CAPACITY      = 4, /* caller-provided capacity too small */
    SNK_ERR_NOT_CONFIGURED = 5,
    SNK_ERR_TIMEOUT       = 6  /* snk_frontend_collect: no frame arrived within the time given */
} snk_status;

/* "infinite" Hamming distance: the Snake side initialises its running minima with 256
 * (Snake/Tracking/SnakeORBMatcher.cpp:121,280,462) and an absent neighbour is reported so. */
#define SNK_DIST_INF 256

SNK_API const char* snk_last_error(void);  /* thread-local text of the last failure */
SNK_API const char* snk_version(void);
SNK_API int snk_device_count(void);        /* number of visible HIP devices (0 = none) */
SNK_API int snk_debug_live_buffers(void);  /* device and pinned scratch buffers all handles of this process hold right now (leak checks) */
SNK_API int snk_debug_buffer_allocations(void); /* such buffers allocated so far, never decreasing: it moves when a call grew a buffer */

/* Run-time switches for choices this library had to DEFINE because the arithmetic lives in the absent saiga submodule
 * (reference .gitmodules:1-3): a maintainer who can read saiga selects the matching rule without editing a kernel.
 * Process-wide, read by every later call; also settable at start-up with SNK_DEFINITIONS="key=value,key=value".
 *   "bf_filter.threshold_strict"  Saiga::BruteForceMatcher::filterMatches(th, ratio), call site
 *                                 Snake/Tracking/TrackingCoarse.cpp:352: 0 = keep d1 <= th (default), 1 = keep d1 < th
 *   "bf_filter.ratio_strict"      same call: 0 = keep d1 <= ratio * d2 (default), 1 = keep d1 < ratio * d2
 *   "iround.mode"                 Saiga::iRound as Preprocess::StereoMatching uses it (Snake/Preprocess/Preprocess.cpp:155,165):
 *                                 0 = floor(x + 0.5) (default), 1 = round half away from zero, 2 = round half to even
 *   "orb.response"                the corner measure of Saiga::ORBExtractor::Detect (ctor call Snake/Preprocess/FeatureDetector.cpp:31-41;
 *                                 the extractor itself is in saiga): 0 = the FAST-9 score (default; published ORB-SLAM2), 1 = the Harris
 *                                 response of the FAST corners (7 x 7 block, k = 0.04: OpenCV's ORB HARRIS_SCORE form).  Under 1 the
 *                                 FAST stage (corners, non-maximum suppression, thresholds, candidate budgets) is unchanged; the Harris
 *                                 response picks the point a quadtree node keeps and is KeyPoint::response.
 * Unknown key / out-of-range value: SNK_ERR_INVALID_ARG, nothing changes.  The oracle mirrors every key (orc_set_definition). */
SNK_API int snk_set_definition(const char* key, int value);
SNK_API int snk_get_definition(const char* key, int* value);

/* ------------------------------------------------------------------------------------------
 * Descriptor matching
 * ------------------------------------------------------------------------------------------ */

/* A rectified / undistorted keypoint as the matchers consume it.  Mirrors the fields of
 * Saiga::KeyPoint<double> that Snake reads: .point, .angle (degrees, float), .octave
 * (Snake/Preprocess/Preprocess.cpp:129-130,214-215; Snake/Map/Features.cpp:24,44). */
typedef struct snk_kp64
{
    double x, y;
    float angle;
    int32_t octave;
} snk_kp64;

/* kNN-2 result for one query descriptor: {idx1, dist1, idx2, dist2}; idx = -1 / dist =
 * SNK_DIST_INF when the train set has fewer than 1 / 2 entries.  A train descriptor at distance
 * 256 (all bits differ) is never reported: 256 is "infinite" on the Snake side. */
typedef struct snk_knn2
{
    int32_t idx1, dist1, idx2, dist2;
} snk_knn2;

typedef struct snk_matcher snk_matcher;

/* device: HIP device ordinal.  stream: a hipStream_t to enqueue on, or NULL for a stream
 * owned by the handle. */
SNK_API int snk_matcher_create(int device, void* stream, snk_matcher** out);
SNK_API int snk_matcher_destroy(snk_matcher* m);
SNK_API int snk_matcher_sync(snk_matcher* m); /* hipStreamSynchronize on the handle's stream */

/* Replaces Saiga::BruteForceMatcher<DescriptorORB>::matchKnn2 / matchKnn2_omp —
 * call site Snake/Tracking/TrackingCoarse.cpp:350-351 (also LoopClosing/LoopORBMatcher.cpp:103-105,
 * Tracking/Initialization/MonoInitializer.cpp:589-592).  For every query the two nearest train
 * descriptors by Hamming distance, ties resolved towards the lower train index. */
SNK_API int snk_bf_knn2(snk_matcher* m, const uint64_t (*query)[4], int nq, const uint64_t (*train)[4], int nt,
                        snk_knn2* out /* nq */);

/* Replaces BruteForceMatcher::filterMatches(threshold, ratio) + the public `matches` vector —
 * Snake/Tracking/TrackingCoarse.cpp:352,373-387.  Keeps (query, idx1) when dist1 <= threshold and
 * dist1 <= ratio * dist2 (float compare), in ascending query order.  pairs has room for nq entries. */
SNK_API int snk_bf_filter(snk_matcher* m, const snk_knn2* knn, int nq, int threshold, float ratio,
                          int32_t (*pairs)[2], int* n_pairs);

/* Batched, device-resident forms.  Layout: batch b owns rows [b*cap, b*cap + n[b]) of each array;
 * counts live on the device (they are produced there by the extractor).  n_pairs_dev[b] receives
 * the number of pairs of batch b. */
SNK_API int snk_bf_knn2_batch_dev(snk_matcher* m, const uint64_t* query_dev, const int32_t* nq_dev, int nq_cap,
                                  const uint64_t* train_dev, const int32_t* nt_dev, int nt_cap, int batch,
                                  snk_knn2* out_dev);
SNK_API int snk_bf_filter_batch_dev(snk_matcher* m, const snk_knn2* knn_dev, const int32_t* nq_dev, int nq_cap,
                                    int batch, int threshold, float ratio, int32_t* pairs_dev /* [batch][nq_cap][2] */,
                                    int32_t* n_pairs_dev);

/* Replaces Snake::Preprocess::StereoMatching(Frame&) — Snake/Preprocess/Preprocess.cpp:122-242
 * (declared Snake/Preprocess/Preprocess.h:33).  left / right are the RECTIFIED keypoints
 * (rect_left.Forward / rect_right.Forward already applied, Preprocess.cpp:140-150); left is in
 * feature-grid order, right in extractor order (Preprocess.cpp:41-49).  level_scale[o] =
 * scalePyramid.Scale(o) (float), n_levels entries.  bf = rect_left.bf.  relaxed =
 * settings.fd_relaxed_stereo.  right_points / depth are in/out (pre-filled with -1000 by
 * Frame::allocateTmp, Snake/Map/Frame.cpp:25-26); only matched entries are overwritten.
 * *n_matches receives the return value of StereoMatching. */
SNK_API int snk_stereo_match(snk_matcher* m, const snk_kp64* left, const uint64_t (*desc_left)[4], int nl,
                             const snk_kp64* right, const uint64_t (*desc_right)[4], int nr, double bf,
                             const float* level_scale, int n_levels, int relaxed, float* right_points, float* depth,
                             int* n_matches);

SNK_API int snk_stereo_match_batch_dev(snk_matcher* m, const snk_kp64* left_dev, const uint64_t* desc_left_dev,
                                       const int32_t* nl_dev, int nl_cap, const snk_kp64* right_dev,
                                       const uint64_t* desc_right_dev, const int32_t* nr_dev, int nr_cap, int batch,
                                       double bf, const float* level_scale_host, int n_levels, int relaxed,
                                       float* right_points_dev, float* depth_dev, int32_t* n_matches_dev);

/* ------------------------------------------------------------------------------------------
 * ORB extractor
 * ------------------------------------------------------------------------------------------ */

/* Constructor arguments of Saiga::ORBExtractor / ORBExtractorGPU as Snake passes them
 * (Snake/Preprocess/FeatureDetector.cpp:31-33,40-41: fd_features, fd_scale_factor, fd_levels,
 * fd_iniThFAST, fd_minThFAST; the CPU extractor's thread count has no meaning here).
 * level_cap bounds the FAST candidates considered per pyramid level (0 = 8192; a power of two
 * in [256, 8192]); see DESIGN.md "candidate budget". */
typedef struct snk_orb_params
{
    int32_t nfeatures;
    float scale_factor;
    int32_t n_levels;
    int32_t ini_th_fast;
    int32_t min_th_fast;
    int32_t level_cap;
} snk_orb_params;

/* Saiga::KeyPoint<float> fields (Snake reads .point, .octave, .angle; FeatureDetector.cpp:129-132). */
typedef struct snk_keypoint
{
    float x, y;     /* level-0 pixel coordinates */
    float size;     /* 31 * scale(octave) */
    float angle;    /* degrees, [0, 360] */
    float response; /* FAST corner score */
    int32_t octave;
} snk_keypoint;

typedef struct snk_orb snk_orb;

SNK_API int snk_orb_create(const snk_orb_params* params, int device, void* stream, snk_orb** out);
SNK_API int snk_orb_destroy(snk_orb* o);
SNK_API int snk_orb_sync(snk_orb* o);

/* Size the device buffers for width x height images and up to max_batch images per call.
 * snk_orb_detect (re)configures itself on the first image / a size change. */
SNK_API int snk_orb_configure(snk_orb* o, int width, int height, int max_batch);
/* Upper bound of keypoints per image for the configured size (output capacity to provide). */
SNK_API int snk_orb_max_keypoints(const snk_orb* o, int* out);

/* Replaces ORBExtractor::Detect / ORBExtractorGPU::Detect(ImageView<uchar>, vector<KeyPoint<float>>&,
 * vector<DescriptorORB>&) — Snake/Preprocess/FeatureDetector.cpp:119,124,149,154.  One synchronous
 * call per image; keypoints and descriptors are index-aligned (FeatureDetector.cpp:169). */
SNK_API int snk_orb_detect(snk_orb* o, const uint8_t* img, int width, int height, int pitch_bytes, snk_keypoint* kps,
                           uint64_t (*desc)[4], int capacity, int* n_out);

/* Batched, device-resident form: image b starts at images_dev + b*image_stride (row pitch
 * pitch_bytes); outputs kps_dev[b*out_cap ...], desc_dev[(b*out_cap + i)*4 ...], n_dev[b].
 * Every image must span pitch_bytes * height readable bytes (image_stride >= that): rows are
 * read in aligned 4-byte units, so up to 3 bytes of a row's padding right of `width` may be
 * read (never used).  Base, pitch and stride that are multiples of 4 take the fast path. */
SNK_API int snk_orb_detect_batch_dev(snk_orb* o, const uint8_t* images_dev, int pitch_bytes, size_t image_stride,
                                     int batch, snk_keypoint* kps_dev, uint64_t* desc_dev, int32_t* n_dev,
                                     int out_cap);

/* Optional per-stage timing with HIP events recorded on the handle's stream around the kernel
 * stages of every detect call: ms[0] = the per-level streaming passes (blurred level + next pyramid
 * level in one pass; plus the stand-alone resize when scale_factor > 2), ms[1] = reserved (the
 * blur used to be a stage of its own; now ~0), ms[2] = FAST cells, ms[3] = distribution,
 * ms[4] = descriptors.  With snk_orb_set_chains(o, 2) a batch of >= 8 images runs as two half-batch
 * launch chains on two streams; each chain is timed on its own stream and counts as one entry of
 * n_calls ("launch chains"), so ms[k] / n_calls is the average duration of one launch and the images
 * per launch are (images processed) / n_calls.
 * snk_orb_stage_times synchronises, returns the summed milliseconds per stage over the launch chains
 * since the last query (ms[5]) and their number, and resets the accumulation. */
SNK_API int snk_orb_set_profiling(snk_orb* o, int enable);

/* Launch chains per snk_orb_detect_batch_dev call (1..4, default 1; environment SNK_ORB_PARTS sets the
 * default).  With more than one chain a batch of >= 8 images is split into equal parts whose kernel
 * sequences run on the handle's stream and on streams owned by the handle, forked from and joined on
 * the handle's stream with events, so the caller-visible ordering is unchanged.  Measured on MI355X:
 * 2 chains +3 % frames/s (the tail of one chain's launch overlaps the other chain), 3-4 chains slower;
 * per-kernel durations are no longer additive.  No reference counterpart. */
SNK_API int snk_orb_set_chains(snk_orb* o, int chains);
/* Staggered schedule of a batch (>= 2 * parts images): the batch is cut into `parts` (2..16; 0 = off) ranges, the front halves
 * (pyramid / blur passes, FAST cells -- bound by vector-instruction issue) run back to back on the handle's stream and the back
 * half of range p (distribution, descriptors -- bound by LDS / cache latency) on a second stream beside the front half of range
 * p + 1.  Same results; the per-kernel times of snk_orb_stage_times then overlap. */
SNK_API int snk_orb_set_stagger(snk_orb* o, int parts);
SNK_API int snk_orb_stage_times(snk_orb* o, float* ms, int* n_calls);

/* Intermediate results of the last call (tests / debugging); no counterpart in the reference — the stages are
 * those of the absent Saiga::ORBExtractor behind Snake/Preprocess/FeatureDetector.cpp:119. */
enum
{
    SNK_ORB_DEBUG_PYRAMID         = 1, /* u8 rows of the level (level >= 1), `pitch` bytes each */
    SNK_ORB_DEBUG_CELL_COUNTS     = 2, /* u16 per FAST cell */
    SNK_ORB_DEBUG_CELL_CANDIDATES = 3, /* u32[64] per cell: score<<12 | (63-dy)<<6 | (63-dx), strongest first */
    SNK_ORB_DEBUG_SELECTED        = 4, /* u32 per slot: x | y<<16 (level pixels) */
    SNK_ORB_DEBUG_SELECTED_COUNT  = 5, /* int */
    SNK_ORB_DEBUG_LEVEL_INFO      = 6, /* int[8]: w, h, pitch, ncols, nrows, wcell, hcell, nfeat */
    SNK_ORB_DEBUG_DIST_QUEUE      = 7  /* int[1 + n]: n, then image * 16 + level of every level the last batched call handed to the
                                          full-budget launch of the distribution (image / level arguments ignored) */
};
SNK_API int snk_orb_debug_fetch(snk_orb* o, int what, int image, int level, void* out, size_t cap_bytes,
                                size_t* n_bytes);

/* ------------------------------------------------------------------------------------------
 * Preprocess: undistort / rectify keypoints
 * ------------------------------------------------------------------------------------------ */

/* The fields of Saiga::Rectification that Snake uses (rect_left / rect_right,
 * Snake/System/SnakeGlobal.h:107-108; filled by Snake/Preprocess/StereoTransforms.cpp:58-68).
 * D_src is the rational radial-tangential model in the order k1 k2 k3 k4 k5 k6 p1 p2. */
typedef struct snk_rectification
{
    double K_src[4]; /* fx fy cx cy */
    double D_src[8];
    double R[9];     /* row-major 3x3 */
    double K_dst[4]; /* fx fy cx cy */
    double bf;
} snk_rectification;

/* Replaces the per-keypoint body of Snake::Preprocess::undistortKeypoints
 * (Snake/Preprocess/Preprocess.cpp:55-77) and Rectification::Forward as applied in
 * StereoMatching (Preprocess.cpp:140-150): out[i] = rectified pixel position with angle / octave
 * copied, normalized[i] = the point stored in frame.normalized_points (may be NULL). */
SNK_API int snk_rectify(snk_matcher* m, const snk_rectification* rect, const snk_keypoint* kps, int n, snk_kp64* out,
                        double (*normalized)[2]);
SNK_API int snk_rectify_batch_dev(snk_matcher* m, const snk_rectification* rect, const snk_keypoint* kps_dev,
                                  const int32_t* n_dev, int cap, int batch, snk_kp64* out_dev, double* normalized_dev);

/* Replaces Snake::Preprocess::ComputeStereoFromRGBD(Frame&) -- Snake/Preprocess/Preprocess.cpp:79-120, the RGB-D branch of
 * Preprocess::Process (:43-46).  The globals it reads (Snake/System/SnakeGlobal.h): K (fx fy cx cy of the undistorted image),
 * rgbd_intrinsics.depthModel.dis (D_depth, rational radial-tangential order k1..k6 p1 p2), rgbd_intrinsics.depthModel.K (K_depth)
 * and rgbd_intrinsics.bf. */
typedef struct snk_rgbd_model
{
    double K[4];
    double D_depth[8];
    double K_depth[4];
    double bf;
} snk_rgbd_model;

/* undistorted = frame.undistorted_keypoints (n), depth_image = frame.depth_image (float metres, row pitch in floats).  Per keypoint:
 * unproject with K, distort with D_depth, project with K_depth, nearest pixel `(int)(v + 0.5)`; depth > 0: depth[i] = depth,
 * right_points[i] = x - bf / depth; else both -1 (:106-114).  *n_matches = the function's return value.  Where the reference aborts
 * (SAIGA_ASSERT: outside the depth image, depth < 0 or >= 20, :100-104) the call returns SNK_ERR_INVALID_ARG with
 * *n_matches = -(index + 1) of the first such keypoint and leaves the outputs untouched.  The _batch_dev form never fails for data:
 * status_dev[b] = 0x7FFFFFFF (fine) or index + 1 of the first offending keypoint (that frame's outputs are then partial). */
SNK_API int snk_rgbd_stereo(snk_matcher* m, const snk_rgbd_model* model, const snk_kp64* undistorted, int n, const float* depth_image,
                            int width, int height, int pitch_floats, float* right_points, float* depth, int* n_matches);
SNK_API int snk_rgbd_stereo_batch_dev(snk_matcher* m, const snk_rgbd_model* model, const snk_kp64* undistorted_dev, const int32_t* n_dev,
                                      int cap, int batch, const float* depth_images_dev, int width, int height, int pitch_floats,
                                      size_t image_stride_floats, float* right_points_dev, float* depth_dev, int32_t* n_matches_dev,
                                      int32_t* status_dev);

/* ------------------------------------------------------------------------------------------
 * Feature grid and projection-guided tracking matchers
 * ------------------------------------------------------------------------------------------ */

/* Saiga::FeatureGridBounds2<double, 20> as Snake uses it (featureGridBounds,
 * Snake/System/SnakeGlobal.h:115): the extent of the undistorted image; 20-px cells. */
typedef struct snk_grid_bounds
{
    double min_x, min_y, max_x, max_y;
} snk_grid_bounds;

/* Replaces frame.grid.create(featureGridBounds, undistorted_keypoints) —
 * Snake/Preprocess/Preprocess.cpp:246: perm[i] = new index of feature i (the caller scatters its
 * arrays as at :254-260); cell_start[cols*rows + 1] = first feature of every cell, cells ordered
 * x-major (id = cx*rows + cy, the order Features::GetFeaturesInArea walks them,
 * Snake/Map/Features.cpp:17-21). */
SNK_API int snk_feature_grid(snk_matcher* m, const snk_kp64* undistorted, int n, const snk_grid_bounds* bounds,
                             int32_t* perm, int32_t* cell_start, int* cols, int* rows);

/* Batched, device-resident Preprocess::computeFeatureGrid (Preprocess.cpp:244-266): builds the grid
 * of every image and scatters its rectified keypoints and descriptors into grid order
 * (kps_out / desc_out); perm_dev [batch][cap], cell_start_dev [batch][cols*rows + 1].
 * n_dev[b] is a device-side count that the host cannot validate: it is read as min(max(n_dev[b], 0), cap), and
 * entries of perm / kps_out / desc_out past that count are left as they were. */
SNK_API int snk_feature_grid_batch_dev(snk_matcher* m, const snk_grid_bounds* bounds, const snk_kp64* kps_dev,
                                       const uint64_t* desc_dev, const int32_t* n_dev, int cap, int batch,
                                       snk_kp64* kps_out_dev, uint64_t* desc_out_dev, int32_t* perm_dev,
                                       int32_t* cell_start_dev);

/* ------------------------------------------------------------------------------------------
 * One stereo frame through the front-end in one call
 * ------------------------------------------------------------------------------------------ */

/* What FeatureDetector + Preprocess are constructed with (Snake/Preprocess/FeatureDetector.cpp:31-41: the extractor arguments;
 * Snake/System/SnakeGlobal.h:107-108,115: rect_left / rect_right, featureGridBounds; Snake/System/Settings.h:123: fd_relaxed_stereo). */
typedef struct snk_frontend_params
{
    snk_orb_params orb;
    snk_rectification rect_left, rect_right; /* undistortKeypoints uses rect_left, StereoMatching's Forward of the right keypoints rect_right */
    snk_grid_bounds bounds;                  /* featureGridBounds */
    double bf;                               /* rect_left.bf / stereo_cam.bf as StereoMatching reads it (Preprocess.cpp:137) */
    int32_t relaxed_stereo;                  /* settings.fd_relaxed_stereo */
    int32_t stereo;                          /* 1 = settings.inputType == Stereo (left + right image, StereoMatching); 0 = mono: left only */
} snk_frontend_params;

/* The members of Snake::Frame that FeatureDetector::Detect and Preprocess::Process fill (Snake/Map/Frame.h, Features.h), as
 * caller-owned arrays of `capacity` entries each (any pointer may be NULL = not wanted).  After the call the left arrays are in
 * FEATURE-GRID order (Preprocess::computeFeatureGrid scatters keypoints, descriptors, undistorted_keypoints and
 * normalized_points, Preprocess.cpp:254-260), the right arrays in extractor order (Preprocess.cpp:41-49). */
typedef struct snk_frontend_frame
{
    int32_t capacity;                 /* in: entries per array (snk_frontend_max_keypoints) */
    int32_t n, n_right, n_stereo;     /* out: frame.N, keypoints_right.size(), the return value of StereoMatching */
    int32_t cols, rows;               /* out: the grid's cell counts (cell id = cx * rows + cy) */
    snk_keypoint* keypoints;          /* frame.keypoints (the reference widens them to KeyPoint<double>; same values) */
    uint64_t (*descriptors)[4];       /* frame.descriptors */
    snk_kp64* undistorted_keypoints;  /* frame.undistorted_keypoints (.point, .angle, .octave) */
    double (*normalized_points)[2];   /* frame.normalized_points */
    int32_t* permutation;             /* what frame.grid.create returned: new index of extractor feature i */
    int32_t* cell_start;              /* cols * rows + 1 entries: first feature of every cell */
    float* right_points;              /* frame.right_points (-1000 where unmatched, Frame.cpp:25) */
    float* depth;                     /* frame.depth (-1000 where unmatched, Frame.cpp:26) */
    snk_keypoint* keypoints_right;    /* frame.keypoints_right */
    uint64_t (*descriptors_right)[4]; /* frame.descriptors_right */
} snk_frontend_frame;

typedef struct snk_frontend snk_frontend;

/* One handle = the reference's FeatureDetector + Preprocess pair for one camera rig: its own stream, extractor and scratch. */
SNK_API int snk_frontend_create(const snk_frontend_params* params, int device, snk_frontend** out);
SNK_API int snk_frontend_destroy(snk_frontend* f);
/* Capacity to provide for images of this size (configures the handle for it). */
SNK_API int snk_frontend_max_keypoints(snk_frontend* f, int width, int height, int* out);
SNK_API int snk_frontend_grid_dims(const snk_frontend* f, int* cols, int* rows);

/* FeatureDetector::Detect (left, right: Snake/Preprocess/FeatureDetector.cpp:116-156) + Preprocess::Process (allocateTmp,
 * undistortKeypoints, computeFeatureGrid, StereoMatching: Snake/Preprocess/Preprocess.cpp:35-53) for ONE frame in ONE synchronous
 * call: one upload of the two images, the extractor as one two-image launch chain, rectification / grid / StereoMatching enqueued
 * behind it, one download, one synchronisation; from the second frame of an image size on the launch sequence is replayed as
 * a hipGraph.  Results are bit for bit those of snk_orb_detect x 2 + snk_rectify x 2 + snk_feature_grid + snk_stereo_match (the same
 * kernels).  level_scale of StereoMatching = the extractor's own pyramid scales (scale[l] = scale[l - 1] * scale_factor in
 * float).  right / pitch_right are ignored by a mono handle.  SNK_ERR_CAPACITY (n / n_right set) when capacity is too small. */
SNK_API int snk_frontend_process(snk_frontend* f, const uint8_t* left, int pitch_left, const uint8_t* right, int pitch_right,
                                 int width, int height, snk_frontend_frame* out);

/* The same frame work PIPELINED, mirroring the reference's blocking single-slot stage queues (SynchronizedSlot<FramePtr>
 * output_buffer: Snake/Preprocess/FeatureDetector.h:39 between FeatureDetection and Preprocess, Preprocess.h:36 between Preprocess and
 * Tracking): the handle owns `depth` independent slots (stream, extractor, scratch, pinned staging, hipGraph, completion event; default 3,
 * snk_frontend_set_depth 1..8 while nothing is in flight).
 *   snk_frontend_submit   stages the images, enqueues upload -> launch chain -> download on the next slot's stream and RETURNS;
 *                         blocks only while all `depth` slots hold uncollected frames (SynchronizedSlot::set).
 *   snk_frontend_collect  waits for the OLDEST submitted frame and fills `out` exactly as snk_frontend_process would (frames
 *                         come back in submission order; bit-identical results).  timeout_ms < 0: wait for a submission as
 *                         long as it takes (SynchronizedSlot::get), 0: do not wait, > 0: that long; SNK_ERR_TIMEOUT when none came.
 *                         SNK_ERR_CAPACITY consumes the frame.
 * One thread may submit while another collects (the reference's FeatureDetection / Preprocess threads); at most one thread on
 * each side.  snk_frontend_process must not be mixed with frames in flight (SNK_ERR_INVALID_ARG); all frames in flight have
 * one image size. */
SNK_API int snk_frontend_set_depth(snk_frontend* f, int depth);
SNK_API int snk_frontend_submit(snk_frontend* f, const uint8_t* left, int pitch_left, const uint8_t* right, int pitch_right,
                                int width, int height);
SNK_API int snk_frontend_collect(snk_frontend* f, snk_frontend_frame* out, int timeout_ms);
SNK_API int snk_frontend_in_flight(snk_frontend* f, int* n);
/* Waits (like snk_frontend_collect: timeout_ms < 0 / 0 / > 0, SNK_ERR_TIMEOUT) until a submitted frame EXISTS -- not until it is
 * finished -- and reports the image size it was submitted with and the capacity its arrays need; the frame stays queued.  This is
 * how a collecting thread sizes its arrays without looking at what the submitting thread is doing (any pointer may be NULL). */
SNK_API int snk_frontend_peek(snk_frontend* f, int timeout_ms, int* width, int* height, int* capacity);
/* snk_frontend_submit without the host-side staging copy (about half of a submit's host time): the upload reads the CALLER's
 * buffers, which must be page-locked (snk_pinned_alloc, hipHostMalloc, hipHostRegister) for the copy to be asynchronous and must
 * stay valid and unmodified until the frame has been collected -- the reference's Input thread owns its image buffers the same
 * way (Snake/Preprocess/Input.h:48, FeatureDetector.h:39).  Rows keep the caller's pitch on the device when pitch_left is a
 * multiple of 4, equals pitch_right and does not exceed the width rounded up to 64 (one copy when right == left + pitch * height,
 * two otherwise); other pitches go through a 2-D copy per image.  Results are bit for bit those of snk_frontend_submit. */
SNK_API int snk_frontend_submit_pinned(snk_frontend* f, const uint8_t* left, int pitch_left, const uint8_t* right, int pitch_right,
                                       int width, int height);
/* Page-locked host memory for the images of snk_frontend_submit_pinned (hipHostMalloc / hipHostFree), for callers that do not link HIP. */
SNK_API int snk_pinned_alloc(size_t bytes, void** out);
SNK_API int snk_pinned_free(void* p);

/* The per-frame data the tracking matchers read (Snake/Map/Features.h:18-41, Frame.h:44-46), in
 * feature-grid order.  taken[i] != 0 <=> frame.mvpMapPoints[i] != nullptr. */
typedef struct snk_frame_view
{
    int32_t n;
    int32_t cols, rows;
    const snk_kp64* kps; /* undistorted_keypoints */
    const uint64_t (*desc)[4];
    const float* right_points;
    const uint8_t* taken;
    const int32_t* cell_start;
    snk_grid_bounds bounds;
} snk_frame_view;

/* K (fx fy cx cy) and stereo_cam.bf (Snake/System/SnakeGlobal.h:103-104). */
typedef struct snk_camera
{
    double fx, fy, cx, cy, bf;
} snk_camera;

/* CoarseTrackingPoint / FineTrackingPoint without the MapPoint* (Snake/Map/LocalMap.h:17-55). */
typedef struct snk_lm_coarse
{
    double pos[3], normal[3];
    uint64_t desc[4];
    int32_t octave;
    float angle;
} snk_lm_coarse;

typedef struct snk_lm_fine
{
    double pos[3], normal[3];
    uint64_t desc[4];
    float reference_depth;
    int32_t reference_scale_level;
    uint8_t valid; /* in/out: cleared by the frustum / distance / viewing-angle culls */
    uint8_t pad[7];
} snk_lm_fine;

/* The Tracking thread looks at one frame with 1-2 coarse calls and one fine call (TrackingCoarse.cpp:234,
 * TrackingFine.cpp:149): snk_match_bind_frame uploads the frame view ONCE and keeps it bound to the handle; the matchers
 * that take a `const snk_frame_view* frame` (snk_match_project_coarse / _fine / _keyframe, snk_match_fuse,
 * snk_match_triangulation_project's frame2; not snk_match_relink, which validates its queries against the view)
 * called with frame == NULL then use the bound frame instead of uploading a view per call.  The view's arrays may be changed or freed after the call.  frame == NULL unbinds. */
SNK_API int snk_match_bind_frame(snk_matcher* m, const snk_frame_view* frame);
/* New `taken` mask (n bytes) for the bound frame: mvpMapPoints changed between two matcher calls. */
SNK_API int snk_match_bound_taken(snk_matcher* m, const uint8_t* taken);

/* Replaces SnakeORBMatcher::SearchByProjectionFrameFrame2 — Snake/Tracking/SnakeORBMatcher.cpp:191-354
 * (call site Snake/Tracking/TrackingCoarse.cpp:234).  pose = CurrentFrame.Pose() (qx qy qz qw tx ty tz).
 * direction: 0 none, 1 bForward, 2 bBackward (:210-212).  match_idx[i] = feature matched to
 * local-map point i or -1 (the adaptor sets mvpMapPoints[match_idx[i]] = lm.points[i].mp);
 * *n_matches = the function's return value. */
SNK_API int snk_match_project_coarse(snk_matcher* m, const snk_frame_view* frame, const snk_camera* cam,
                                     const double pose[7], const snk_lm_coarse* pts, int n_pts, float th, int feature_error,
                                     int direction, const float* level_scale, int n_levels, int32_t* match_idx,
                                     int* n_matches);

/* Replaces SnakeORBMatcher::SearchByProjection2 — Snake/Tracking/SnakeORBMatcher.cpp:365-526 (call
 * site Snake/Tracking/TrackingFine.cpp:149).  pts[i].valid is updated like lmp.valid; visible[i] = 1
 * where the reference calls lmp.mp->IncreaseVisible() (:431). */
SNK_API int snk_match_project_fine(snk_matcher* m, const snk_frame_view* frame, const snk_camera* cam, const double pose[7],
                                   snk_lm_fine* pts, int n_pts, float th, float ratio, const float* level_scale, int n_levels,
                                   int32_t* match_idx, uint8_t* visible, int* n_matches);

/* Device-resident, batched forms of the two per-frame tracking matchers: frame b of the batch is what the batched
 * front-end leaves in HBM -- keypoints and descriptors in feature-grid order and cell_start
 * (snk_feature_grid_batch_dev), right_points (snk_stereo_match_batch_dev) -- so the matchers consume it without a
 * host round trip.  All per-feature arrays are [batch][cap]; cell_start is [batch][cols * rows + 1] for the 20-px grid
 * of `bounds`; taken[b][i] != 0 <=> mvpMapPoints[i] != nullptr (all zero for a fresh frame; snk_match_mark_taken_batch_dev
 * applies the adaptor's `mvpMapPoints[idx] = mp` between the coarse and the fine call). */
typedef struct snk_frames_dev
{
    int32_t batch, cap;
    const int32_t* n;           /* [batch] features per frame */
    const snk_kp64* kps;        /* [batch][cap] undistorted keypoints, grid order */
    const uint64_t* desc;       /* [batch][cap][4] */
    const float* right_points;  /* [batch][cap] */
    const uint8_t* taken;       /* [batch][cap] */
    const int32_t* cell_start;  /* [batch][cols * rows + 1] */
    snk_grid_bounds bounds;
} snk_frames_dev;

/* SearchByProjectionFrameFrame2 for every frame of the batch (same rules and results as snk_match_project_coarse).
 * poses_dev: [batch][7] doubles ON THE DEVICE (qx qy qz qw tx ty tz; e.g. left there by the previous frame's pose
 * refinement); pts_dev [batch][pts_cap], n_pts_dev [batch]; outputs match_idx_dev [batch][pts_cap] (-1 = none, also for
 * entries past n_pts) and n_matches_dev [batch].  Asynchronous on the handle's stream.
 * The device-side counts cannot be validated by the host, so every batched entry below (coarse, fine, fine_ro, mark_taken) reads
 * n_pts_dev[b] as min(max(n_pts_dev[b], 0), pts_cap) and frames->n[b] as min(max(n[b], 0), cap): a count out of range gives the
 * results of the clamped count and no access outside the frame's rows. */
SNK_API int snk_match_project_coarse_batch_dev(snk_matcher* m, const snk_frames_dev* frames, const snk_camera* cam,
                                               const double* poses_dev, const snk_lm_coarse* pts_dev,
                                               const int32_t* n_pts_dev, int pts_cap, float th, int feature_error,
                                               int direction, const float* level_scale, int n_levels,
                                               int32_t* match_idx_dev, int32_t* n_matches_dev);

/* SearchByProjection2 (SnakeORBMatcher.cpp:365-526) for every frame of the batch (same rules and results as snk_match_project_fine; pts_dev[..].valid is
 * updated in place, visible_dev [batch][pts_cap]). */
SNK_API int snk_match_project_fine_batch_dev(snk_matcher* m, const snk_frames_dev* frames, const snk_camera* cam,
                                             const double* poses_dev, snk_lm_fine* pts_dev, const int32_t* n_pts_dev,
                                             int pts_cap, float th, float ratio, const float* level_scale, int n_levels,
                                             int32_t* match_idx_dev, uint8_t* visible_dev, int32_t* n_matches_dev);

/* The same with the local-map records READ-ONLY: pts_dev[..].valid is read, never written.  The flag the reference leaves in lmp.valid
 * (SnakeORBMatcher.cpp:397-428) is visible_dev[b][i]: a point keeps valid = 1 exactly when it passes every cull, which is where
 * IncreaseVisible() is called (:431).  For callers that match a local map again (or share its records between frames) without restoring
 * it, and 6 x fewer bytes written: the in-place flag is one byte into each 96-byte record. */
SNK_API int snk_match_project_fine_batch_ro_dev(snk_matcher* m, const snk_frames_dev* frames, const snk_camera* cam,
                                                const double* poses_dev, const snk_lm_fine* pts_dev, const int32_t* n_pts_dev,
                                                int pts_cap, float th, float ratio, const float* level_scale, int n_levels,
                                                int32_t* match_idx_dev, uint8_t* visible_dev, int32_t* n_matches_dev);

/* taken_dev[b][match_idx_dev[b][i]] = 1 for every matched point: `CurrentFrame.mvpMapPoints[idx] = mp`
 * (SnakeORBMatcher.cpp:330, :522) applied on the device between two matcher calls on the same frames. */
SNK_API int snk_match_mark_taken_batch_dev(snk_matcher* m, const int32_t* match_idx_dev, const int32_t* n_pts_dev, int pts_cap,
                                           int batch, uint8_t* taken_dev, int cap);

/* Replaces SnakeORBMatcher::SearchByProjectionFrameToKeyframe — Snake/Tracking/SnakeORBMatcher.cpp:71-188.
 * positions / descriptors: mp->getPosition() / mp->GetDescriptor() of kf.GetMapPointMatches();
 * skip[i] != 0 where the keyframe has no point or the frame already holds it (:102-103).
 * Greedy and sequential like the reference: a feature given to point i is unavailable to i+1. */
SNK_API int snk_match_project_keyframe(snk_matcher* m, const snk_frame_view* frame, const snk_camera* cam,
                                       const double pose[7], const double (*positions)[3],
                                       const uint64_t (*descriptors)[4], const uint8_t* skip, int n_pts, float th,
                                       int feature_error, int32_t* match_idx, int* n_matches);

/* ------------------------------------------------------------------------------------------
 * Keyframe-rate matchers of local mapping
 * ------------------------------------------------------------------------------------------ */

/* FusionPoint, all fields (Snake/Map/LocalMap.h:57-80). */
typedef struct snk_fusion_point
{
    double pos[3], normal[3];
    uint64_t desc[4];
    float reference_depth;
    int32_t reference_scale_level;
    int32_t observations;
    int32_t id;
} snk_fusion_point;

/* Replaces MappingORBMatcher::Fuse(kf, pose, point_mask, LocalMap<FusionPoint>, fuseCandidates, th,
 * obs_factor, feature_th) — Snake/LocalMapping/MappingORBMatcher.cpp:359-480 (call sites
 * Snake/LocalMapping/NeighbourSearch.cpp:177,188).  frame = kf->frame (grid order; `taken` unused),
 * point_mask may be NULL.  best_idx[i] = keyframe feature point i would be fused into, or -1; the
 * caller emplaces (best_idx[i], pts[i].id) in point order.  *n_fused = the return value. */
SNK_API int snk_match_fuse(snk_matcher* m, const snk_frame_view* frame, const snk_camera* cam, const double pose[7],
                           const snk_fusion_point* pts, const uint8_t* point_mask, int n_pts, float th, float obs_factor,
                           int feature_th, const float* level_scale, int n_levels, int32_t* best_idx, int* n_fused);

/* Replaces MappingORBMatcher::SearchForTriangulationProject — MappingORBMatcher.cpp:168-249 (call
 * site Snake/LocalMapping/Triangulator.cpp:170).  depth_grid: row-major [grid_rows][grid_cols], one
 * depth per 4 x 4 feature-grid cells (:194-195); kps1 / np1 / desc1 / has_mp1: keyframe 1
 * (undistorted_keypoints, normalized_points, descriptors, GetMapPoint(i) != nullptr), any order;
 * frame2: keyframe 2 in grid order with taken[i] = GetMapPoint(i) != nullptr, np2 its
 * normalized_points; E12 row-major.  Saiga::EpipolarDistanceSquared (absent) is [DEFINED] as the
 * squared distance of np2 to the line E12 * (np1, 1).  match_idx2[i] = feature of keyframe 2 paired
 * with feature i of keyframe 1, or -1. */
SNK_API int snk_match_triangulation_project(snk_matcher* m, const double* depth_grid, int grid_rows, int grid_cols,
                                            const double pose1[7], const double pose2[7], const snk_camera* cam,
                                            const snk_kp64* kps1, const double (*np1)[2], const uint64_t (*desc1)[4],
                                            const uint8_t* has_mp1, int n1, const snk_frame_view* frame2,
                                            const double (*np2)[2], const double E12[9], float epipolar_distance,
                                            int feature_distance, int32_t* match_idx2, int* n_matches);

/* frame->bow_feature_vec (an ordered map vocabulary node -> feature indices, filled by the reference's
 * bag-of-words transform) flattened: node_id strictly ascending, node_start[n_nodes + 1] offsets into
 * `features`, each node's features in the order the reference iterates them. */
typedef struct snk_bow_features
{
    int32_t n_nodes;
    int32_t pad;
    const uint32_t* node_id;
    const int32_t* node_start;
    const int32_t* features;
} snk_bow_features;

/* Replaces MappingORBMatcher::SearchForTriangulation2 — Snake/LocalMapping/MappingORBMatcher.cpp:14-99
 * (call site Snake/LocalMapping/Triangulator.cpp:164).  np / desc / has_mp: normalized_points,
 * descriptors, GetMapPoint(i) != nullptr of each keyframe (any order; the bag-of-words vectors index
 * them).  pairs must hold bow1->node_start[n_nodes] entries; it receives (idx1, idx2) in the order the
 * reference emplaces them; *n_matches = the return value.  tmp_flags of the reference is never set
 * (:26-27, :59), so a keyframe-2 feature may be paired with several keyframe-1 features, as there. */
SNK_API int snk_match_triangulation_bow(snk_matcher* m, const snk_camera* cam, const double E12[9], const double (*np1)[2],
                                        const uint64_t (*desc1)[4], const uint8_t* has_mp1, int n1,
                                        const snk_bow_features* bow1, const double (*np2)[2], const uint64_t (*desc2)[4],
                                        const uint8_t* has_mp2, int n2, const snk_bow_features* bow2,
                                        float epipolar_distance, int feature_distance, int32_t (*pairs)[2], int* n_matches);

/* Replaces MappingORBMatcher::SearchForTriangulationBF — MappingORBMatcher.cpp:102-165: all pairs,
 * epipolar gate of 10 px (:107; the reference ignores its epipolarDistance argument), then the
 * descriptor gate.  match_idx2[i] = feature of keyframe 2 paired with feature i of keyframe 1, or -1. */
SNK_API int snk_match_triangulation_bf(snk_matcher* m, const snk_camera* cam, const double E12[9], const double (*np1)[2],
                                       const uint64_t (*desc1)[4], const uint8_t* has_mp1, int n1, const double (*np2)[2],
                                       const uint64_t (*desc2)[4], const uint8_t* has_mp2, int n2, int feature_distance,
                                       int32_t* match_idx2, int* n_matches);

/* One (keyframe feature, map point) observation of DeferredMapper::Relink — Snake/Optimizer/DeferredMapper.cpp:61-99. */
typedef struct snk_relink_query
{
    double pos[3];        /* mp->getPosition() */
    uint64_t desc[4];     /* mp->descriptor */
    uint64_t alt_desc[4]; /* descriptor of mp's first observation in another keyframe (:90-98), if has_alt */
    int32_t feature;      /* i: the feature of the keyframe that holds mp (grid order) */
    int32_t has_alt;
} snk_relink_query;

#define SNK_RELINK_KEEP 0
#define SNK_RELINK_ERASE 1  /* behind the camera or reprojection error > outlier_threshold (:75-81) */
#define SNK_RELINK_MOVE 2   /* best_idx = a closer feature with a strictly better descriptor (:101-138) */

/* Replaces the per-observation search of DeferredMapper::Relink — Snake/Optimizer/DeferredMapper.cpp:39-165
 * (call site :32); reference constants: radius 0.8, outlier_threshold = reprojectionErrorThresholdMono
 * = 2.1, feature_threshold 25 (:41-43).  frame = kf->frame (grid order; `taken` unused), pose =
 * kf->Pose().  The map edits stay on the caller's side, in feature order as in the reference: ERASE ->
 * EraseMapPointMatch / EraseObservation; MOVE -> if kf->GetMapPoint(best_idx) is a good point at that
 * moment erase (:143-152) else relink (:155-161).  A point moved to a LATER feature is visited again
 * by the reference's loop with its recomputed descriptor: the caller queries it again (n = 1).
 * stereo_cam.LeftPointToRight(x, z) (absent saiga) is [DEFINED] as x - bf / z.
 * *n_changed = number of queries with action != KEEP. */
SNK_API int snk_match_relink(snk_matcher* m, const snk_frame_view* frame, const snk_camera* cam, const double pose[7],
                             const snk_relink_query* queries, int n, float radius, double outlier_threshold,
                             int feature_threshold, int32_t* action, int32_t* best_idx, int* n_changed);

/* ------------------------------------------------------------------------------------------
 * New map points from matched keyframe pairs (semantics "snk-tri v1")
 * ------------------------------------------------------------------------------------------ */

/* One keyframe as the loop of Triangulator::triangulate reads it — Snake/LocalMapping/Triangulator.cpp:135-138,
 * :176-185, :204-206: kf->frame->undistorted_keypoints / right_points (>= 0 <=> stereo) / depth, has_mp[i] != 0 <=>
 * kf->GetMapPoint(i) != nullptr (:67), pose = kf->Pose() (qx qy qz qw tx ty tz, world -> camera).  Any feature order;
 * n <= 65536. */
typedef struct snk_tri_view
{
    int32_t n;
    int32_t pad;
    const snk_kp64* kps;
    const float* right_points;
    const float* depth;
    const uint8_t* has_mp;
    double pose[7];
} snk_tri_view;

/* TriangulationParams::errorMono / errorStereo (Triangulator.cpp:127-128), the global th_depth (:225,:230),
 * scalePyramid.Factor() (:132) and settings.inputType == InputType::Mono (:142). */
typedef struct snk_tri_params
{
    float error_mono, error_stereo;
    double th_depth;
    float scale_factor;
    int32_t mono;
} snk_tri_params;

#define SNK_TRI_TRIANGULATED 1 /* Triangulator.cpp:215-221 */
#define SNK_TRI_STEREO1 2      /* :222-226: unprojected with keyframe 1's stereo depth */
#define SNK_TRI_STEREO2 3      /* :227-231 */

/* ImageTriangulationResult::NewPoint (Triangulator.cpp:284-290) plus what the commit loop needs: `neighbour` = index of kf2
 * in the call, `branch` = which of the three constructions made the point (SNK_TRI_*), `commit` = 1 where the loop of
 * :61-108 reaches allocateMapPoint for this entry (the test of :67 is false when the entry is visited). */
typedef struct snk_new_point
{
    int32_t feature1, feature2; /* featureId1, featureId2 */
    int32_t neighbour;
    uint8_t far_away;
    uint8_t commit;
    uint8_t branch;
    uint8_t pad;
    double pos[3]; /* worldPosition */
} snk_new_point;

/* Replaces the geometric loop of Triangulator::triangulate for ONE keyframe pair — Snake/LocalMapping/Triangulator.cpp:127-157
 * (chi-square thresholds, ratioFactor, the baseline gate) and :174-291 (parallax test, TriangulateHomogeneous, the stereo
 * fallbacks, behind-camera / chi-square / scale-consistency gates).  pairs = tmp_matches (idx1, idx2) after the matchers of
 * :164-171; out (capacity n_pairs) receives result.newPoints in pair order, *n_out their number.  median_depth2 =
 * kf2->MedianDepth() (:145), read in mono mode only.  commit is set as the loop of :61-70 would for this pair alone: from
 * has_mp of both views and the earlier kept entries of this call.  Absent saiga functions are [DEFINED]: stereo_cam.baseLine()
 * = bf / fx, K.unproject(p, z) = ((x - cx) / fx * z, (y - cy) / fy * z, z), projectStereo(X) = (u, v, u - bf / z),
 * SquaredScale(o) = level_scale[o]^2, TriangulateHomogeneous = unit-row homogeneous linear system, smallest right singular
 * vector.  A feature index outside [0, n), an octave outside [0, n_levels) or a NULL array with a non-zero count:
 * SNK_ERR_INVALID_ARG, nothing is launched.  n_pairs == 0 is valid. */
SNK_API int snk_triangulate_pairs(snk_matcher* m, const snk_camera* cam, const snk_tri_params* params, const snk_tri_view* kf1,
                                  const snk_tri_view* kf2, float median_depth2, const int32_t (*pairs)[2], int n_pairs,
                                  const float* level_scale, int n_levels, snk_new_point* out, int* n_out);

/* The whole neighbour loop of Triangulator::Process — Snake/LocalMapping/Triangulator.cpp:42-47 — plus the first-wins test of
 * its commit loop (:61-70) in one call: kf2s[k] = tmp_keyframes[k], pairs = every neighbour's tmp_matches concatenated,
 * pair_start[n_neighbours + 1] their offsets (pair_start[0] = 0).  out (capacity pair_start[n_neighbours]) receives
 * newPointsa[0].newPoints, newPointsa[1].newPoints, ... back to back, out_start[n_neighbours + 1] the offsets of each
 * neighbour's points, *n_out = out_start[n_neighbours].  commit: the entries are visited in that order; one is kept iff
 * kf1->GetMapPoint(feature1) and kf2->GetMapPoint(feature2) are both still null at that moment, i.e. has_mp is 0 for both and
 * no earlier kept entry used feature1 of keyframe 1 or feature2 of the same neighbour.  (Neighbours must be distinct
 * keyframes, as GetBestCovisibilityKeyFrames returns them.)  The map edits of :72-106 stay with the caller, for the entries
 * with commit = 1, in order.  n_neighbours == 0 and empty pair lists are valid and launch nothing. */
SNK_API int snk_triangulate_neighbours(snk_matcher* m, const snk_camera* cam, const snk_tri_params* params, const snk_tri_view* kf1,
                                       const snk_tri_view* kf2s, const float* median_depth2s, int n_neighbours,
                                       const int32_t (*pairs)[2], const int32_t* pair_start, const float* level_scale, int n_levels,
                                       snk_new_point* out, int32_t* out_start, int* n_out);

/* ------------------------------------------------------------------------------------------
 * Map-point refresh: descriptor, normal, reference depth (semantics "snk-mp v1")
 * ------------------------------------------------------------------------------------------ */

#define SNK_MP_MAX_OBS 4096 /* observations of one point: 128 KiB of descriptors in a workgroup's LDS (160 KiB per CU) */

#define SNK_MP_MEDIAN 0 /* m(i) = element (N - 1) / 2 of row i of the distance matrix, sorted ascending: the ORB-SLAM rule */
#define SNK_MP_SUM 1    /* m(i) = sum of row i */

#define SNK_MP_DESCRIPTOR 1 /* MapPoint::ComputeDistinctiveDescriptors, Snake/Map/MapPoint.cpp:60-81 */
#define SNK_MP_NORMAL 2     /* MapPoint::UpdateNormal, :120-135 */
#define SNK_MP_DEPTH 4      /* MapPoint::UpdateDepth, :154-166 */

#define SNK_MP_OK 0
#define SNK_MP_BAD_INDEX 1 /* device form: a (kf_slot, feature), a ref_obs or an obs_start outside its range */
#define SNK_MP_TOO_MANY 2  /* device form: more than SNK_MP_MAX_OBS observations */

typedef struct snk_mp_params
{
    int32_t rule; /* SNK_MP_MEDIAN / SNK_MP_SUM */
    int32_t what; /* SNK_MP_DESCRIPTOR | SNK_MP_NORMAL | SNK_MP_DEPTH */
} snk_mp_params;

/* One refreshed point.  A part that `what` does not select, or that the rules leave untouched, has best = -1 and desc = 0
 * (descriptor), normal = (0, 0, 0), ref_level = -1 and ref_depth = 0; n_valid is always the number of valid observations.
 * status != SNK_MP_OK (device form only): every other field has those values and n_valid = 0. */
typedef struct snk_mp_result
{
    int32_t best;      /* bestId of MapPoint.cpp:79 as an index into the point's full list (invalid entries included); -1: none */
    int32_t n_valid;   /* N */
    int32_t ref_level; /* reference_scale_level, :165 */
    int32_t status;
    double normal[3];  /* :134 */
    double ref_depth;  /* reference_depth, :162 */
    uint64_t desc[4];  /* descriptor, :80 */
} snk_mp_result;

/* MapPoint::ComputeDistinctiveDescriptors, UpdateNormal and UpdateDepth — Snake/Map/MapPoint.cpp:60-81, :120-135, :154-166 —
 * for n_points map points in one call, as the reference's loops gather them (Triangulator.cpp:94-97, LocalMapping.cpp:179,215,
 * NeighbourSearch.cpp:218-219, LocalBundleAdjustment.cpp:497, ...).  Point p owns the observations obs_start[p] ..
 * obs_start[p + 1] - 1 (obs_start[0] = 0) in the order of mObservations; per observation: desc = frame->descriptors[obs.second]
 * (:72), cam_pose = obs.first->Pose() (qx qy qz qw tx ty tz, world -> camera; CameraPosition() = -R^T t, :128), octave =
 * undistorted_keypoints[obs.second].octave (:165), valid != 0 <=> !obs.first->isBad() (:71, :127).  Per point: position and
 * ref_obs = indexInternal(referenceKF) as an index into the point's list (-1: UpdateDepth is not run for it).  out[n_points].
 * The rules are [DEFINED] (Saiga::MeanMatcher and Eigen are absent): invalid observations are skipped; the descriptor is the first
 * valid observation in list order whose row of Hamming distances to all valid ones (itself included) has the smallest median
 * (element (N - 1) / 2 of the sorted row) or sum; the normal is the sum in list order of the unit vectors towards the camera
 * centres, normalised (a zero vector stays zero), all in fp64 without contraction; ref_depth = |position - C_ref|.  The results
 * do not depend on the kernel form (SNK_MP_FORM=packed|wide forces one, read once).
 * A NULL array with a non-zero count, a non-monotone obs_start, a ref_obs outside [-1, k), a point with more than SNK_MP_MAX_OBS
 * observations, an unknown rule or `what` bit: SNK_ERR_INVALID_ARG, nothing is launched.  n_points == 0 and points with k = 0 are
 * valid. */
SNK_API int snk_mappoint_refresh(snk_matcher* m, const snk_mp_params* params, int n_points, const int32_t* obs_start,
                                 const uint64_t (*desc)[4], const double (*cam_pose)[7], const int32_t* octave, const uint8_t* valid,
                                 const double (*position)[3], const int32_t* ref_obs, snk_mp_result* out);

/* The same refresh (MapPoint.cpp:60-81, :120-135, :154-166) with everything resident on the device: the keyframes are the slots
 * of `frames` (desc and kps [batch][cap] as the batched front-end leaves them; right_points / taken / cell_start are not read)
 * with poses_dev [batch][7]; observation o is obs_dev[o] = (kf_slot, feature) with valid_dev[o]; obs_start_dev [n_points + 1]
 * indexes obs_dev [n_obs]; position_dev [n_points][3], ref_obs_dev [n_points]; out_dev [n_points].  Asynchronous on the handle's
 * stream, no host round trip.  Nothing can be checked on the host, so the kernels check: a point with an obs_start outside
 * [0, n_obs] or decreasing, a ref_obs outside [-1, k), or a valid (or reference) observation outside [0, batch) x [0, n[slot]) gets
 * status = SNK_MP_BAD_INDEX, one with k > SNK_MP_MAX_OBS gets SNK_MP_TOO_MANY, and nothing outside those ranges is read. */
SNK_API int snk_mappoint_refresh_batch_dev(snk_matcher* m, const snk_mp_params* params, const snk_frames_dev* frames,
                                           const double* poses_dev, int n_points, const int32_t* obs_start_dev, int n_obs,
                                           const int32_t (*obs_dev)[2], const uint8_t* valid_dev, const double* position_dev,
                                           const int32_t* ref_obs_dev, snk_mp_result* out_dev);

/* ------------------------------------------------------------------------------------------
 * Covisibility: connection lists and the local-keyframe vote (semantics "snk-covis v1")
 * ------------------------------------------------------------------------------------------ */

#define SNK_COVIS_MAX_KF 32768 /* keyframe slots: a u32 counter per keyframe is 128 KiB of a compute unit's 160 KiB LDS */
#define SNK_COVIS_MAX_CAP 4096 /* list entries kept per set: their ids are sorted in 16 KiB of LDS beside the counters */

#define SNK_COVIS_OK 0
#define SNK_COVIS_UNCHANGED 1 /* no keyframe touched: the reference returns and leaves the old connections (Keyframe.cpp:125-129) */
#define SNK_COVIS_BAD_INDEX 2 /* device forms: a query, a start, a point id or an observation's keyframe outside its range */

#define SNK_COVIS_PT_BAD 1 /* pt_flags bit 0: !(*mp) / mp->isBad() */
#define SNK_COVIS_PT_FAR 2 /* pt_flags bit 1: mp->far_stereo_point */

/* The map as tables, keyframe slots 0 .. n_kf - 1, point ids 0 .. n_points - 1.  Host pointers for snk_covis_update / snk_covis_vote,
 * device pointers for the _batch_dev forms.  The two sides of the map (obs here, feat_point of the calls) are read as given. */
typedef struct snk_covis_map
{
    int32_t n_kf, n_points, n_obs;
    const uint8_t* kf_bad;      /* [n_kf] Keyframe::isBad() */
    const int32_t* obs_start;   /* [n_points + 1], obs_start[0] = 0 */
    const int32_t (*obs)[2];    /* [n_obs] mp->GetObservationList() in list order as (kf, feature): the layout of snk_mappoint_refresh_batch_dev */
    const uint8_t* pt_flags;    /* [n_points] SNK_COVIS_PT_BAD | SNK_COVIS_PT_FAR */
} snk_covis_map;

typedef struct snk_covis_params
{
    int32_t th;     /* Keyframe.cpp:135: 15.  >= 1.  The vote has no threshold but checks the field alike */
    float th_depth; /* Keyframe.cpp:111.  Not read by the vote */
    int32_t cap;    /* entries of conn per set, 1 .. SNK_COVIS_MAX_CAP */
} snk_covis_params;

typedef struct snk_covis_conn
{
    int32_t weight;
    int32_t kf;
} snk_covis_conn;

/* One set.  The list is ascending by (weight, kf); n_found is its full length, n_conn = min(n_found, cap) entries are in conn[set]
 * [0 .. n_conn): the LAST n_conn of the list, still ascending (every consumer reads from the back); entries past n_conn are not
 * written.  best_kf = the last entry (-1: empty list).  status != SNK_COVIS_OK: n_found = n_conn = 0, best_kf = -1. */
typedef struct snk_covis_result
{
    int32_t n_found;
    int32_t n_conn;
    int32_t best_kf;
    int32_t status;
} snk_covis_result;

/* Keyframe::UpdateConnections — Snake/Map/Keyframe.cpp:89-171 — for the n_q keyframes q[0 .. n_q) in one call, every query against
 * the same tables (UpdateConnections changes connections, not observations; the caller applies the lists in order).  Keyframe k owns
 * the features feat_start[k] .. feat_start[k + 1] - 1 (feat_start[n_kf + 1], feat_start[0] = 0): feat_point = observations[i] as a point
 * id (-1: none), feat_depth = frame->depth[i].  A feature counts unless its point is bad (:107), far or deeper than th_depth (:111;
 * equality and depths <= 0 count); every observation (k, .) of its point with k != q adds 1 to count[k] (:117-121), duplicates as
 * often as they occur, bad keyframes included.  Nothing touched: SNK_COVIS_UNCHANGED (:125).  The list is every touched keyframe that is
 * not bad (:141) with count >= th (:147); if none, the one with the largest count (:154), [DEFINED] the smallest id among equals; only
 * bad ones touched: an empty list with SNK_COVIS_OK.  Order [DEFINED]: ascending by (weight, kf), the order KeyframeGraph.cpp:124
 * keeps.  best_kf is the parent candidate of :168; GetBestCovisibilityKeyFrames(N) (KeyframeGraph.cpp:62) is the last N entries.
 * AddConnection on the listed keyframes (:150,157) and the parent / child links (:166-170) stay with the caller.
 * conn [n_q][cap], out [n_q].  Everything is checked before anything is launched: a NULL array with a non-zero count, a start array that
 * does not begin at 0 or decreases, an id outside its range, n_kf > SNK_COVIS_MAX_KF, cap outside [1, SNK_COVIS_MAX_CAP], th < 1:
 * SNK_ERR_INVALID_ARG.  n_q == 0, keyframes without features and points without observations are valid.  The results do not
 * depend on the kernel form (SNK_COVIS_LONG_MIN=<n> moves the length from which a wavefront walks a list, read once). */
SNK_API int snk_covis_update(snk_matcher* m, const snk_covis_map* map, const int32_t* feat_start, const int32_t* feat_point,
                             const float* feat_depth, const snk_covis_params* params, int n_q, const int32_t* q, snk_covis_conn* conn,
                             snk_covis_result* out);

/* The same (Keyframe.cpp:89-171) with every table, q_dev, conn_dev and out_dev on the device; n_feat is the length of feat_point_dev /
 * feat_depth_dev.  Asynchronous on the handle's stream, no host round trip.  n_kf, cap and th are checked on the host; the host
 * cannot look at the tables, so the kernel checks: a query outside [0, n_kf), a feature range outside [0, n_feat] or decreasing, a
 * point id >= n_points or < -1, an obs_start outside [0, n_obs] or decreasing, an observation's keyframe outside [0, n_kf) give that
 * set status = SNK_COVIS_BAD_INDEX, and nothing outside the ranges is read. */
SNK_API int snk_covis_update_batch_dev(snk_matcher* m, const snk_covis_map* map_dev, const int32_t* feat_start_dev, int n_feat,
                                       const int32_t* feat_point_dev, const float* feat_depth_dev, const snk_covis_params* params, int n_q,
                                       const int32_t* q_dev, snk_covis_conn* conn_dev, snk_covis_result* out_dev);

/* The vote at the head of Tracking::UpdateLocalKeyFrames2 — Snake/Tracking/TrackingFine.cpp:230-268 — for n_sets frames: set s is
 * the point ids set_point[set_start[s] .. set_start[s + 1]) (a frame's mvpMapPoints, -1 = none, so a padded [batch][cap] array with
 * set_start[b] = b * cap is a valid input).  -1 and bad points are skipped (:233-239); every observation adds 1 to its keyframe
 * (:241-251): no self exclusion, no depth gate, no threshold, bad keyframes are kept.  The list is every touched keyframe ascending by
 * (count, id) (:267, [DEFINED] the id for the pointer), best_kf = reference_keyframe (:268); nothing touched: SNK_COVIS_UNCHANGED
 * (:254).  Clearing the bad points of the frame (:237) and everything from :272 on stay with the caller.  Of params only cap has an
 * effect.  Checks and errors as snk_covis_update (th < 1 included). */
SNK_API int snk_covis_vote(snk_matcher* m, const snk_covis_map* map, int n_sets, const int32_t* set_start, const int32_t* set_point,
                           const snk_covis_params* params, snk_covis_conn* conn, snk_covis_result* out);

/* The same vote (TrackingFine.cpp:230-268) on the device; n_set_points is the length of set_point_dev.  Asynchronous, checked by the
 * kernel as snk_covis_update_batch_dev checks: a set range outside [0, n_set_points] or decreasing, a point id, an obs_start or an
 * observation's keyframe outside its range give status = SNK_COVIS_BAD_INDEX. */
SNK_API int snk_covis_vote_batch_dev(snk_matcher* m, const snk_covis_map* map_dev, int n_sets, const int32_t* set_start_dev,
                                     int n_set_points, const int32_t* set_point_dev, const snk_covis_params* params,
                                     snk_covis_conn* conn_dev, snk_covis_result* out_dev);

/* ------------------------------------------------------------------------------------------
 * Local BA windows (snk-scene v1)
 * ------------------------------------------------------------------------------------------ */

#define SNK_SCENE_MAX_WINDOW 64    /* n_neighbours + 1 + n_last at most, win_cap at most */
#define SNK_SCENE_MAX_IMG 4096     /* [DEFINED] img_cap at most */
#define SNK_SCENE_MAX_OBS 4194304  /* [DEFINED] obs_cap at most */

#define SNK_SCENE_OK 0
#define SNK_SCENE_SKIPPED 1         /* the query keyframe is bad (LocalBundleAdjustment.cpp:77) */
#define SNK_SCENE_WINDOW_OVERFLOW 2 /* more than win_cap window keyframes */
#define SNK_SCENE_PTS_OVERFLOW 3    /* more than pt_cap distinct points */
#define SNK_SCENE_IMG_OVERFLOW 4    /* more than img_cap images */
#define SNK_SCENE_OBS_OVERFLOW 5    /* more than obs_cap observation records */
#define SNK_SCENE_BAD_INDEX 6       /* device forms: an id, a start or a count outside its range */

#define SNK_SCENE_PT_CONST 4 /* pt_flags bit 2: mp->constant (beside SNK_COVIS_PT_BAD, SNK_COVIS_PT_FAR) */

struct snk_ba_rpc; /* defined with the bundle adjustment below */

/* The map as tables: the layouts and names of snk_covis_map / snk_lmap_map where they exist.  Host pointers for snk_scene_gather, device
 * pointers for the _batch_dev form.  The IMU tables are either all NULL (no constraints) or all present. */
typedef struct snk_scene_map
{
    int32_t n_kf, n_points, n_obs, n_feat, n_levels;
    const uint8_t* kf_bad;           /* [n_kf] */
    const int32_t* kf_prev;          /* [n_kf] previousKF as a slot, -1: none.  Not read by snk_scene_gather */
    const double* kf_pose;           /* [n_kf][7] world -> camera: qx qy qz qw tx ty tz */
    const int32_t* feat_start;       /* [n_kf + 1], feat_start[0] = 0 */
    const int32_t* feat_point;       /* [n_feat] point ids, -1: none */
    const float* feat_depth;         /* [n_feat] frame->depth[i] */
    const float* feat_uv;            /* [n_feat][2] undistorted_keypoints[i].point */
    const int32_t* feat_octave;      /* [n_feat] undistorted_keypoints[i].octave, 0 .. n_levels - 1 */
    const int32_t* obs_start;        /* [n_points + 1], obs_start[0] = 0 */
    const int32_t (*obs)[2];         /* [n_obs] GetObservationList() in list order as (kf, feature index inside the keyframe) */
    const uint8_t* pt_flags;         /* [n_points] SNK_COVIS_PT_BAD | SNK_SCENE_PT_CONST */
    const double* pt_pos;            /* [n_points][3] */
    const float* level_inv_sq_scale; /* [n_levels] scalePyramid.InverseSquaredScale */
    const double* kf_time;           /* [n_kf] frame->timeStamp */
    const double* kf_imu_begin;      /* [n_kf] imudata.time_begin */
    const double* kf_imu_end;        /* [n_kf] imudata.time_end */
    const uint8_t* kf_preint_valid;  /* [n_kf] */
    const struct snk_ba_rpc* kf_rpc; /* [n_kf] kf->rpc: only rel_pose and weight_translation are read */
} snk_scene_map;

typedef struct snk_scene_params
{
    int32_t n_neighbours; /* :126: 15 */
    int32_t n_last;       /* :132: 20.  n_neighbours + 1 + n_last <= SNK_SCENE_MAX_WINDOW */
    double gyro_weight;   /* current_gyro_weight: constraints only if > 0 and the IMU tables are present */
    double acc_weight;    /* current_acc_weight */
} snk_scene_params;

/* One query of snk_scene_window.  status != SNK_SCENE_OK: n_window = 0. */
typedef struct snk_scene_window_result
{
    int32_t n_window;
    int32_t status;
} snk_scene_window_result;

/* One query of snk_scene_gather.  status != SNK_SCENE_OK: all counts 0. */
typedef struct snk_scene_result
{
    int32_t n_window; /* the first n_window images are the window keyframes (constant = 0) */
    int32_t n_img, n_pt, n_obs, n_rpc;
    int32_t status;
} snk_scene_result;

/* The outputs of snk_scene_gather, row s for query s, laid out as snk_ba_problem takes them.  Rows past a query's counts are not
 * written, except pt_id, which is -1 past n_pt (all of it where status != SNK_SCENE_OK). */
typedef struct snk_scene_out
{
    int32_t win_cap, pt_cap, img_cap, obs_cap;
    int32_t* img_kf;         /* [n_q][img_cap] kfmapinv */
    double* pose;            /* [n_q][img_cap][7] */
    uint8_t* img_const;      /* [n_q][img_cap] */
    int32_t* pt_id;          /* [n_q][pt_cap] mpmapinv */
    double* pt;              /* [n_q][pt_cap][3] */
    uint8_t* pt_const;       /* [n_q][pt_cap] */
    uint8_t* pt_valid;       /* [n_q][pt_cap] wp.valid = nEdges > 0 (:292) */
    int32_t* obs_img;        /* [n_q][obs_cap] */
    int32_t* obs_pt;         /* [n_q][obs_cap] */
    double* obs_uv;          /* [n_q][obs_cap][2] */
    double* obs_depth;       /* [n_q][obs_cap] */
    double* obs_weight;      /* [n_q][obs_cap] */
    int32_t* obs_src;        /* [n_q][obs_cap][2] (kf, feature index inside the keyframe): where an outlier flag goes in the map */
    struct snk_ba_rpc* rpc;  /* [n_q][win_cap]; may be NULL where no constraints can be emitted */
    snk_scene_result* result; /* [n_q] */
} snk_scene_out;

/* The window of LocalBundleAdjustment::MakeLocalScene — Snake/Optimizer/LocalBundleAdjustment.cpp:124-151 — for the n_q keyframes
 * q[0 .. n_q).  conn_start [n_kf + 1] / conn_list are every keyframe's connections ascending by (weight, kf), the arguments of
 * snk_lmap_select.  Candidates: the last min(n_neighbours, size) connections of q, q itself, then k = kf_prev[q], kf_prev[k], ... for at
 * most n_last steps, stopping at -1; a bad keyframe of the chain counts as a step and is walked through.  Duplicates (:142) and bad
 * keyframes (:145) are dropped, the rest is sorted ascending ([DEFINED] the slot stands for Keyframe::id(), as in snk-covis v1).
 * window_kf [n_q][win_cap] (-1 past n_window), out [n_q].  q bad (:77): SNK_SCENE_SKIPPED; more than win_cap survivors:
 * SNK_SCENE_WINDOW_OVERFLOW.  map.KeyFramesInMap() < 2 (:113) stays with the caller.  Everything is checked before anything is launched: a
 * NULL array with a non-zero count, a start array that does not begin at 0 or decreases, a keyframe outside its range (q, kf_prev
 * outside [-1, n_kf), a connection), n_kf > SNK_COVIS_MAX_KF, win_cap outside [1, SNK_SCENE_MAX_WINDOW], a parameter below 0,
 * n_neighbours + 1 + n_last > SNK_SCENE_MAX_WINDOW: SNK_ERR_INVALID_ARG.  n_q == 0 is valid. */
SNK_API int snk_scene_window(snk_matcher* m, int n_q, const int32_t* q, int n_kf, const uint8_t* kf_bad, const int32_t* kf_prev,
                             const int32_t* conn_start, const snk_covis_conn* conn_list, const snk_scene_params* params, int win_cap,
                             int32_t* window_kf, snk_scene_window_result* out);

/* The same (:124-151) with every array on the device; n_list is the length of conn_list_dev.  Asynchronous on the handle's stream.  The
 * kernel checks what the host cannot see: a query outside [0, n_kf), a kf_prev outside [-1, n_kf), a conn_start range outside
 * [0, n_list] or decreasing, a connection's keyframe outside [0, n_kf) give that query SNK_SCENE_BAD_INDEX (before SKIPPED is looked
 * at only for the query itself), and nothing outside the ranges is read. */
SNK_API int snk_scene_window_batch_dev(snk_matcher* m, int n_q, const int32_t* q_dev, int n_kf, const uint8_t* kf_bad_dev,
                                       const int32_t* kf_prev_dev, const int32_t* conn_start_dev, int n_list,
                                       const snk_covis_conn* conn_list_dev, const snk_scene_params* params, int win_cap,
                                       int32_t* window_kf_dev, snk_scene_window_result* out_dev);

/* The scene of MakeLocalScene — LocalBundleAdjustment.cpp:154-346 — for n_q windows.  window_kf [n_q][out->win_cap] and win [n_q] are
 * what snk_scene_window left; a stage-1 status other than OK is passed through.  Points (:154-167): the window keyframes in order, their
 * features in order, -1 and bad points skipped, first appearances only.  Fixed cameras (:170-184): the points in that order, their
 * observations in list order; every keyframe that is neither bad nor in the window, in order of first appearance.  Images (:200-244):
 * the window (constant 0), then the fixed cameras (constant 1).  World points (:246-254) in point order; pt_valid = the point has an
 * observation by a keyframe that is not bad (:292).  Observation records (:258-291): a bad keyframe's are skipped, so are those whose
 * image and point are both constant; the rest is {image, point, uv, depth, weight = level_inv_sq_scale[octave]} widened to double,
 * ordered as the flattened img.stereoPoints: image by image, inside an image ascending by (point index, list position).  Constraints
 * (:295-346), only with the IMU tables and gyro_weight > 0: consecutive window keyframes (a, b) at images i - 1, i with
 * kf_time[a] == kf_imu_begin[b], kf_time[b] == kf_imu_end[b], kf_preint_valid[b] give {i - 1, i, kf_rpc[b].rel_pose, gyro_weight / dt,
 * kf_rpc[b].weight_translation * acc_weight / dt}, dt = kf_time[b] - kf_time[a], both weights 0 for dt > 2 ([DEFINED] the record's own
 * img1 / img2 are not read).  Overflows are reported in the order PTS, IMG, OBS.  [DEFINED] the observations of a window's points are at
 * most 2^30, its features too.  perKeyframeData / perPointData, stateBefore and UpdateLocalScene stay with the caller.
 * Everything is checked before anything is launched: NULL arrays, caps outside [1, limit] (pt_cap <= SNK_LMAP_MAX_PTS), starts that do
 * not begin at 0 or decrease, a point id outside [-1, n_points), an observation's keyframe outside [0, n_kf) or feature outside its
 * keyframe's range, an octave outside [0, n_levels), a window that is not strictly ascending or out of range, IMU tables partly
 * present: SNK_ERR_INVALID_ARG. */
SNK_API int snk_scene_gather(snk_matcher* m, int n_q, const snk_scene_map* map, const int32_t* window_kf,
                             const snk_scene_window_result* win, const snk_scene_params* params, const snk_scene_out* out);

/* The same (:154-346) with every table and every output on the device.  Asynchronous.  The kernel checks the same and answers
 * SNK_SCENE_BAD_INDEX for that query alone; the range checks of a phase come before its overflow, so a status does not depend on
 * timing.  Only the ranges a query reaches are checked. */
SNK_API int snk_scene_gather_batch_dev(snk_matcher* m, int n_q, const snk_scene_map* map_dev, const int32_t* window_kf_dev,
                                       const snk_scene_window_result* win_dev, const snk_scene_params* params,
                                       const snk_scene_out* out_dev);

/* ------------------------------------------------------------------------------------------
 * Local map of fine tracking (snk-lmap v1)
 * ------------------------------------------------------------------------------------------ */

#define SNK_LMAP_MAX_LOCAL_KF 256  /* kf_cap at most: local keyframes per set */
#define SNK_LMAP_MAX_PTS 16384     /* pts_cap at most (the reference reserves 10 000, LocalMap.h:88): 32 768 four-byte slots of LDS */
#define SNK_LMAP_MAX_NEIGHBOURS 16 /* [DEFINED] n_neighbours at most (the reference asks for 5) */

#define SNK_LMAP_OK 0
#define SNK_LMAP_EMPTY 1        /* the vote touched nothing (TrackingFine.cpp:254): no local keyframes; snk_lmap_gather adds the own points only */
#define SNK_LMAP_TRUNCATED 2    /* the vote's list was cut by its cap (n_found > n_conn): the remaining and the marked keyframes are unknown */
#define SNK_LMAP_KF_OVERFLOW 3  /* more than kf_cap local keyframes */
#define SNK_LMAP_PTS_OVERFLOW 4 /* more than pts_cap distinct points */
#define SNK_LMAP_BAD_INDEX 5    /* device forms: an id, a start or a count outside its range */

typedef struct snk_lmap_params
{
    int32_t n_direct;        /* TrackingFine.cpp:223: 15 */
    int32_t n_direct_prob;   /* :224: 5 */
    int32_t n_indirect_prob; /* :225: 5 */
    int32_t n_neighbours;    /* :301: 5.  0 .. SNK_LMAP_MAX_NEIGHBOURS */
    int32_t kf_cap;          /* entries of local_kf per set, 1 .. SNK_LMAP_MAX_LOCAL_KF */
    uint64_t seed;           /* of the draws; a set's draws depend on (seed, frame_id, position) only */
} snk_lmap_params;

/* One set of snk_lmap_select.  status != SNK_LMAP_OK: n_local = n_direct = n_indirect = 0, reference_kf = -1. */
typedef struct snk_lmap_select_result
{
    int32_t n_local;      /* local_keyframes.size() */
    int32_t n_direct;     /* min(params.n_direct, length of the vote's list) */
    int32_t n_indirect;   /* indirect_neighbor.size(): the rejected of the first walk + the neighbours appended */
    int32_t reference_kf; /* :268 */
    int32_t status;
} snk_lmap_select_result;

/* One set of snk_lmap_gather.  status other than SNK_LMAP_OK / SNK_LMAP_EMPTY: all counts 0. */
typedef struct snk_lmap_gather_result
{
    int32_t n_pts;        /* lm.points.size(), the return value of UpdateLocalPoints */
    int32_t n_searchable; /* records with valid = 1 */
    int32_t n_own_new;    /* own points that no local keyframe placed */
    int32_t status;       /* SNK_LMAP_OK also where stage 1 said SNK_LMAP_EMPTY */
} snk_lmap_gather_result;

/* The keyframe side of the map and the per-point words snk_lmap_gather reads.  n_feat: length of feat_point (host forms: must equal
 * feat_start[n_kf]). */
typedef struct snk_lmap_map
{
    int32_t n_kf, n_points, n_feat;
    const int32_t* feat_start;   /* [n_kf + 1], feat_start[0] = 0: the layout of snk_covis_update */
    const int32_t* feat_point;   /* [n_feat] GetMapPointMatches() as point ids, -1: none */
    const uint8_t* pt_flags;     /* [n_points] bit SNK_COVIS_PT_BAD */
    const int32_t* pt_last_seen; /* [n_points] MapPoint::lastFrameSeen */
} snk_lmap_map;

/* What FineTrackingPoint's constructor copies (LocalMap.h:46-53), a row per point id; e.g. what snk_mappoint_refresh leaves. */
typedef struct snk_lmap_points
{
    const double* pos;        /* [n_points][3] */
    const double* normal;     /* [n_points][3] */
    const uint64_t* desc;     /* [n_points][4] */
    const float* ref_depth;   /* [n_points] */
    const int32_t* ref_level; /* [n_points] */
} snk_lmap_points;

/* The local keyframes of Tracking::UpdateLocalKeyFrames2 behind the vote — Snake/Tracking/TrackingFine.cpp:272-323 — for n_sets
 * frames.  conn [n_sets][vote_cap] and vote [n_sets] are what snk_covis_vote left (ascending by (count, id), read from the back);
 * conn_start [n_kf + 1] / conn_list [conn_start[n_kf]] are every keyframe's connections, ascending by (weight, kf) as snk_covis_update
 * emits them and KeyframeGraph.cpp:124 keeps them.  Vote SNK_COVIS_UNCHANGED: SNK_LMAP_EMPTY (:254); n_found > n_conn:
 * SNK_LMAP_TRUNCATED.  Direct: the last min(n_direct, n_found) entries from the back (:272-276), reference_kf the last (:268).  The
 * remaining R entries from the back (:282-295): entry j takes draw j against n_direct_prob / R; accepted ones join the local list,
 * rejected ones `indirect`.  For every local keyframe so far, in order, the last min(n_neighbours, size) connections in ASCENDING
 * order (KeyframeGraph.cpp:62 is a view): a neighbour that is not bad (:304) and not marked (:306) joins `indirect` and is marked;
 * marked are all keyframes of the vote's list (:246-250) and the neighbours appended.  Entry j of `indirect` takes draw R + j against
 * n_indirect_prob / indirect.size() (:316-323).  Bad keyframes of the vote's list are kept.  Draw c of a set [DEFINED]:
 * h = mix(mix(key) ^ c), key = mix(mix(seed lo ^ 0x9e3779b9) ^ seed hi) ^ frame_id, accepted iff (u64)h * n < (u64)k << 32 (Saiga::Random
 * is absent).  More than kf_cap local keyframes: SNK_LMAP_KF_OVERFLOW.  local_kf [n_sets][kf_cap] (-1 past n_local), out [n_sets].
 * Everything is checked before anything is launched: a NULL array with a non-zero count, a start array that does not begin at 0 or
 * decreases, an id or a vote count outside its range, n_kf > SNK_COVIS_MAX_KF, kf_cap outside [1, SNK_LMAP_MAX_LOCAL_KF], n_neighbours
 * above SNK_LMAP_MAX_NEIGHBOURS, a parameter below 0: SNK_ERR_INVALID_ARG.  n_sets == 0 is valid. */
SNK_API int snk_lmap_select(snk_matcher* m, int n_sets, const snk_covis_conn* conn, int vote_cap, const snk_covis_result* vote, int n_kf,
                            const uint8_t* kf_bad, const int32_t* conn_start, const snk_covis_conn* conn_list, const int32_t* frame_id,
                            const snk_lmap_params* params, int32_t* local_kf, snk_lmap_select_result* out);

/* The same (TrackingFine.cpp:272-323) with every array on the device; n_list is the length of conn_list_dev.  Asynchronous on the
 * handle's stream.  The kernel checks what the host cannot see: a vote record with counts outside [0, vote_cap] or a status it does not
 * know, a keyframe id outside [0, n_kf), a conn_start entry that decreases or lies outside [0, n_list] give that set
 * SNK_LMAP_BAD_INDEX, and nothing outside the ranges is read. */
SNK_API int snk_lmap_select_batch_dev(snk_matcher* m, int n_sets, const snk_covis_conn* conn_dev, int vote_cap,
                                      const snk_covis_result* vote_dev, int n_kf, const uint8_t* kf_bad_dev, const int32_t* conn_start_dev,
                                      int n_list, const snk_covis_conn* conn_list_dev, const int32_t* frame_id_dev,
                                      const snk_lmap_params* params, int32_t* local_kf_dev, snk_lmap_select_result* out_dev);

/* Tracking::UpdateLocalPoints with LocalMap::addPoint — Snake/Tracking/TrackingFine.cpp:328-356, Snake/Map/LocalMap.h:139-154 — for
 * n_sets frames.  local_kf [n_sets][kf_cap] and sel [n_sets] are what snk_lmap_select left.  For every local keyframe in list order and
 * every feature in feature order: a point that is -1, bad or last seen in this frame (pt_last_seen[p] == frame_id[s], :338-339) is
 * skipped, otherwise addPoint: a point already present keeps its first place (also twice inside one keyframe).  Then the frame's own
 * points set_point[set_start[s] .. set_start[s + 1]) (the vote's arrays) in order, -1 and bad skipped: one already present has valid
 * cleared in its record, a new one is appended with valid = 0 (:344-354).  More than pts_cap distinct points: SNK_LMAP_PTS_OVERFLOW.  A
 * stage-1 status other than OK / EMPTY is passed through; EMPTY adds the own points only.  Outputs: lm_pts [n_sets][pts_cap] (pad bytes
 * 0), lm_point [n_sets][pts_cap] point ids (-1 past n_pts; lm.points[i].mp), n_pts [n_sets] -- lm_pts, n_pts plug into
 * snk_match_project_fine_batch_dev / _ro_dev --, out [n_sets]; records past n_pts are not written.  IncreaseVisible on the own points
 * (:349) and clearing the frame's bad points (:237) stay with the caller.  Checks and errors as snk_lmap_select, pts_cap in
 * [1, SNK_LMAP_MAX_PTS]. */
SNK_API int snk_lmap_gather(snk_matcher* m, int n_sets, const snk_lmap_map* map, const snk_lmap_points* points, const int32_t* frame_id,
                            const int32_t* local_kf, int kf_cap, const snk_lmap_select_result* sel, const int32_t* set_start,
                            const int32_t* set_point, int pts_cap, snk_lm_fine* lm_pts, int32_t* lm_point, int32_t* n_pts,
                            snk_lmap_gather_result* out);

/* The same (TrackingFine.cpp:328-356, LocalMap.h:139-154) on the device; n_set_points is the length of set_point_dev.  Asynchronous.
 * The kernel checks: a stage-1 count outside [0, kf_cap], a local keyframe outside [0, n_kf), a feature range outside [0, n_feat] or
 * decreasing, a set range outside [0, n_set_points] or decreasing, a point id >= n_points or < -1, more than 2^30 candidates give that
 * set SNK_LMAP_BAD_INDEX. */
SNK_API int snk_lmap_gather_batch_dev(snk_matcher* m, int n_sets, const snk_lmap_map* map_dev, const snk_lmap_points* points_dev,
                                      const int32_t* frame_id_dev, const int32_t* local_kf_dev, int kf_cap,
                                      const snk_lmap_select_result* sel_dev, const int32_t* set_start_dev, int n_set_points,
                                      const int32_t* set_point_dev, int pts_cap, snk_lm_fine* lm_pts_dev, int32_t* lm_point_dev,
                                      int32_t* n_pts_dev, snk_lmap_gather_result* out_dev);

/* ------------------------------------------------------------------------------------------
 * Pose refinement (the step after every projection matcher)
 * ------------------------------------------------------------------------------------------ */

/* Saiga ObsBase<double> as the reference fills it per match — Snake/Tracking/PoseRefinement.h:47-55,
 * PoseRefinement.cpp:46-52: ip = undistorted keypoint, weight = sqrt(InverseSquaredScale(octave)),
 * depth = frame.depth[i] (> 0 => stereo observation, u_r = u - bf / depth). */
typedef struct snk_pose_obs
{
    double x, y;
    double depth;
    double weight;
} snk_pose_obs;

/* th_mono / th_stereo = reprojectionErrorThreshold{Mono,Stereo} * errorFactor (PoseRefinement.cpp:13-15,
 * Snake/System/SnakeGlobal.h:145-146).  The optimiser the reference calls
 * (Saiga::RobustPoseOptimization::optimizePoseRobust, absent submodule) is [DEFINED] as "snk-pose v1"
 * (DESIGN.md 3c): outer_iterations rounds of inner_iterations damped Gauss-Newton steps over the
 * current inliers, Huber (delta = threshold) in the first robust_rounds rounds, every match
 * re-classified after each round (outlier <=> |r|^2 > threshold^2).  Defaults of the Python / C++
 * mirrors: 4, 10, 3, lambda = 1e-4. */
typedef struct snk_pose_options
{
    double th_mono, th_stereo;
    int32_t outer_iterations, inner_iterations, robust_rounds, pad;
    double lambda;
} snk_pose_options;

/* One frame: wps[i] = position of the map point matched to feature idx[i] (lm.points[lid].position
 * or pMP->getPosition()), obs[i] as above; pose = frame.Pose() in, optimised pose out (world ->
 * camera, qx qy qz qw tx ty tz); outlier[i] -> frame.mvbOutlier[idx[i]]; inliers = the return value
 * of optimizePoseRobust.  prediction / w_rot / w_trans = frame.prediction and
 * frame.prediction_weight_{rotation,translation} (RobustSmoothPoseOptimization branch,
 * PoseRefinement.h:68-73); both weights 0 => no prior. */
typedef struct snk_pose_problem
{
    int32_t n;
    int32_t inliers; /* out */
    const double (*wps)[3];
    const snk_pose_obs* obs;
    uint8_t* outlier; /* out [n] */
    double pose[7];   /* in / out */
    double prediction[7];
    double w_rot, w_trans;
} snk_pose_problem;

/* Replaces rpo.optimizePoseRobust / rpo_smooth.optimizePoseRobust for a batch of frames (one
 * wavefront per frame, one launch).  Host pointers, synchronous. */
SNK_API int snk_pose_refine(snk_matcher* m, const snk_camera* cam, const snk_pose_options* opt,
                            snk_pose_problem* problems, int n_problems);

/* Device-resident PoseRefinement::RefinePoseWithMatches (Snake/Tracking/PoseRefinement.cpp:25-79) for every frame of a batch,
 * fed by the result of a batched projection matcher: for local-map point i with match_idx[b][i] = f >= 0 the pair
 * (world point = 3 doubles at pts_dev + (b * pts_cap + i) * pts_stride -- snk_lm_coarse / snk_lm_fine both start with it --,
 * observation = frames->kps[b][f], depth_dev[b][f] (> 0 => stereo), weight sqrt(InverseSquaredScale(octave))) enters in
 * point order.  poses_dev [batch][7] is the start pose and receives the refined one (untouched with fewer than 3 pairs);
 * outlier_dev [batch][pts_cap] gets the flag of every matched point (0 elsewhere), inliers_dev [batch] the return value.
 * Asynchronous on the handle's stream; with snk_match_project_coarse_batch_dev before and _fine_batch_dev after it a frame's
 * tracking chain (TrackingCoarse.cpp:234-270, TrackingFine.cpp:149-158) runs without a host round trip. */
SNK_API int snk_pose_refine_matches_batch_dev(snk_matcher* m, const snk_frames_dev* frames, const float* depth_dev,
                                              const snk_camera* cam, const snk_pose_options* opt, const void* pts_dev,
                                              int pts_stride, const int32_t* match_idx_dev, const int32_t* n_pts_dev,
                                              int pts_cap, const float* level_scale, int n_levels, double* poses_dev,
                                              uint8_t* outlier_dev, int32_t* inliers_dev);

/* The same refinement fed the way the reference feeds it: frame_pt_dev [batch][frames->cap] is `frame.mvpMapPoints` as indices
 * into the frame's point table (pts_dev [batch][pts_cap] records of pts_stride bytes starting with the position; -1 = nullptr,
 * entries >= n_pts_dev[b] are ignored) and the pairs enter in FEATURE order -- the loop `for (auto i : frame.featureRange())` of
 * PoseRefinement.cpp:37-57.  outlier_dev [batch][frames->cap] is `frame.mvbOutlier` (flag of every feature with a point, 0
 * elsewhere); frames->n is required.  Everything else as snk_pose_refine_matches_batch_dev. */
SNK_API int snk_pose_refine_frame_batch_dev(snk_matcher* m, const snk_frames_dev* frames, const float* depth_dev,
                                            const snk_camera* cam, const snk_pose_options* opt, const void* pts_dev,
                                            int pts_stride, const int32_t* frame_pt_dev, const int32_t* n_pts_dev,
                                            int pts_cap, const float* level_scale, int n_levels, double* poses_dev,
                                            uint8_t* outlier_dev, int32_t* inliers_dev);

/* Several sequences per GPU in lockstep (BASELINE.json config 5, "sequences batched"): the two glue steps that keep frame t of
 * every sequence on the device between the batched BF matcher and the batched pose refinement.
 * snk_track_bf_matches_batch_dev -- Tracking::TrackBruteForce, Snake/Tracking/TrackingCoarse.cpp:342-387: the reference matches
 * `matchKnn2_omp(frame.descriptors, ref->frame->descriptors)` (:351) -- the CURRENT frame is the query set -- and sets
 * `frame.mvpMapPoints[m.first] = ref->GetMapPoint(m.second)` for the filtered matches whose reference feature has a point
 * (:373-377).  pairs_dev [batch][cap][2] = (current feature f, reference feature r), n_pairs_dev [batch]: the output of
 * snk_bf_filter_batch_dev with the current frame as query set; ref_has_dev [batch][cap] = the reference feature has a map point;
 * output frame_pt_dev[b][f] = r for those matches, -1 (nullptr) everywhere else -- mvpMapPoints as indices, the form
 * snk_pose_refine_frame_batch_dev consumes with the reference frame's points as the point table.
 * snk_track_backproject_batch_dev -- the stereo points of every frame in the world, p_w = R^T (p_c - t) with
 * p_c = ((x - cx) / fx * z, (y - cy) / fy * z, z), z = depth (the inverse of `currentPose * wp`,
 * Snake/Tracking/SnakeORBMatcher.cpp:229): world_dev [batch][cap][3], has_dev [batch][cap] = depth > 0.  Both asynchronous on the
 * handle's stream. */
SNK_API int snk_track_bf_matches_batch_dev(snk_matcher* m, const int32_t* pairs_dev, const int32_t* n_pairs_dev,
                                           const uint8_t* ref_has_dev, int cap, int batch, int32_t* frame_pt_dev);
SNK_API int snk_track_backproject_batch_dev(snk_matcher* m, const snk_frames_dev* frames, const float* depth_dev,
                                            const snk_camera* cam, const double* poses_dev, double* world_dev, uint8_t* has_dev);

/* ------------------------------------------------------------------------------------------
 * P3P-RANSAC of TrackBruteForce (semantics "snk-p3p v1")
 * ------------------------------------------------------------------------------------------ */

/* RansacParameters as Tracking::TrackBruteForce sets them -- Snake/Tracking/TrackingCoarse.cpp:410-414: iterations = maxIterations
 * (250), residual_threshold = residualThreshold = (2 * reprojectionErrorThresholdMono / K.fx)^2, a squared distance in the
 * normalised image plane.  `threads` has no meaning here: every hypothesis of every problem of a call runs in one launch.  seed:
 * the sampler is a counter-based hash of (seed, problem index in the call, hypothesis, draw), so a call is a pure function of its
 * arguments. */
typedef struct snk_p3p_params
{
    int32_t iterations;
    int32_t pad;
    double residual_threshold;
    uint64_t seed;
} snk_p3p_params;

/* One call of `pnp2.solve(wps, ips, pose, inlierMatches, inlierMask)` -- TrackingCoarse.cpp:403-440: wps[i] = world point of pair
 * i, nips[i] = K.unproject2(undistorted keypoint) (:383-385); n <= 3072.  Out: pose (world -> camera, qx qy qz qw tx ty tz; left as
 * it came in when n < 4 or no hypothesis has a solution), inliers = the return value, inlier_mask[n], inlier_matches[0 .. inliers)
 * ascending (capacity n), best_iteration / best_solution = the winning hypothesis and the index of the winning pose among that
 * hypothesis' solutions (-1 / -1 without a winner). */
typedef struct snk_p3p_problem
{
    int32_t n;
    int32_t inliers;
    const double (*wps)[3];
    const double (*nips)[2];
    uint8_t* inlier_mask;
    int32_t* inlier_matches;
    double pose[7];
    int32_t best_iteration, best_solution;
} snk_p3p_problem;

/* Replaces P3PRansac::solve for a batch of problems -- Snake/Tracking/TrackingCoarse.cpp:403-440 (call :420): per hypothesis
 * three distinct pairs, the <= 4 poses of the minimal solver, every pose scored against all n pairs (inlier <=> z_c > 0 and
 * |p_c.xy / z_c - nip|^2 < residual_threshold); the winner has the most inliers, ties go to the smaller hypothesis, then to the
 * smaller solution index; no refinement (RefinePoseWithMatches follows at :452).  Host pointers, synchronous, one launch for the
 * batch; the result is identical from run to run.  n_problems == 0 is valid. */
SNK_API int snk_p3p_ransac(snk_matcher* m, const snk_p3p_params* params, snk_p3p_problem* problems, int n_problems);

/* The same for ONE problem with every hypothesis laid open, for tests (TrackingCoarse.cpp:403-440 has no counterpart: the loop is
 * inside P3PRansac): triplets[k] = the three pair indices of hypothesis k, n_solutions[k] in 0..4, poses[k][j] / counts[k][j] = pose
 * and inlier count of its solution j (zeros past n_solutions[k]).  All arrays have params->iterations entries.  `problem` is filled
 * as by snk_p3p_ransac. */
SNK_API int snk_p3p_debug_hypotheses(snk_matcher* m, const snk_p3p_params* params, snk_p3p_problem* problem,
                                     int32_t (*triplets)[3], int32_t* n_solutions, double (*poses)[4][7], int32_t (*counts)[4]);

/* Device-resident form for every frame of a batch, between snk_track_bf_matches_batch_dev and snk_pose_refine_frame_batch_dev and fed
 * like the latter -- Snake/Tracking/TrackingCoarse.cpp:373-440: the pairs of frame b are its features f with
 * 0 <= frame_pt_dev[b][f] < n_pts_dev[b], in feature order (the order of matchesIds, :373-387), world point = 3 doubles at
 * pts_dev + (b * pts_cap + frame_pt_dev[b][f]) * pts_stride, nip = ((x - cx) / fx, (y - cy) / fy) of frames->kps[b][f] (:383-385);
 * problem index = b.  poses_dev [batch][7] receives the winner's pose (untouched without a winner), inliers_dev [batch] the count,
 * and frame_pt_dev[b][f] becomes -1 at every feature that is not an inlier (:433-440: mvpMapPoints keeps the inliers only).
 * frames->cap <= 3072.  Asynchronous on the handle's stream: BF matches -> RANSAC -> refinement without a host round trip. */
SNK_API int snk_p3p_ransac_frame_batch_dev(snk_matcher* m, const snk_frames_dev* frames, const snk_camera* cam,
                                           const snk_p3p_params* params, const void* pts_dev, int pts_stride, int32_t* frame_pt_dev,
                                           const int32_t* n_pts_dev, int pts_cap, double* poses_dev, int32_t* inliers_dev);

/* ------------------------------------------------------------------------------------------
 * Registration RANSAC of the loop detector (semantics "snk-sim3 v1")
 * ------------------------------------------------------------------------------------------ */

/* What LoopDetector::solve sets on its solver -- Snake/LoopClosing/LoopDetector.cpp:152-205: threshold = 12 squared pixels (:156),
 * compute_scale (:231: mono input only), and the iteration count of :203, RansacIterationsFromProbability(N, 0.999, 15, 100) =
 * (probability, min_inliers, max_iterations).  iterations > 0 forces the count; iterations = 0 uses
 * snk_ransac_iterations(n, probability, min_inliers, max_iterations) per problem.  seed: the sampler is the counter-based hash of
 * "snk-p3p v1" over (seed, problem index in the call, hypothesis, draw).  Limits: iterations and max_iterations <= 2^20,
 * 0 < probability < 1, min_inliers >= 1, max_iterations >= 1 (the last three are read only with iterations = 0). */
typedef struct snk_sim3_params
{
    int32_t iterations;
    int32_t compute_scale;
    double threshold;
    uint64_t seed;
    double probability;
    int32_t min_inliers, max_iterations;
} snk_sim3_params;

/* One call of `solver.solve(its, compute_scale)` -- LoopDetector.cpp:152-205: pair i is points1[i] = pose1 * (point of keyframe 1)
 * (:193), points2[i] = pose2 * (its partner of keyframe 2) (:194), ips1[i] / ips2[i] = their undistorted keypoints in pixels
 * (:185-190); cam = K for both views (:158-159; bf is not read); n <= 2048.  Out: T = qx qy qz qw tx ty tz and scale with
 * points2 ~ scale * R * points1 + t (both left as they came in when n < 3 or no hypothesis has an inlier), inliers, inlier_mask[n]
 * (vbInliers, :200-201), best_iteration (-1 without a winner). */
typedef struct snk_sim3_problem
{
    int32_t n;
    int32_t inliers;
    const double (*points1)[3];
    const double (*points2)[3];
    const double (*ips1)[2];
    const double (*ips2)[2];
    uint8_t* inlier_mask;
    snk_camera cam;
    double T[7];
    double scale;
    int32_t best_iteration, pad;
} snk_sim3_problem;

/* RansacIterationsFromProbability of LoopDetector.cpp:203 (the function is in saiga; [DEFINED]): eps = min_inliers / n; 1 when
 * n <= 0 or eps >= 1, else ceil(log(1 - probability) / log(1 - eps^3)) in double, clamped to [1, max_iterations].  Host helper. */
SNK_API int snk_ransac_iterations(int n, double probability, int min_inliers, int max_iterations);

/* Replaces LoopDetector::solve's `solver.solve(its, compute_scale)` for a batch of problems -- LoopDetector.cpp:148-206: per
 * hypothesis three distinct pairs, the similarity (or rigid) transform of the two triplets by Horn's quaternion method, scored
 * against all n pairs by the reprojection error in both images (inlier <=> both points in front of their camera and both squared
 * errors < threshold); the winner has the most inliers, ties go to the smaller hypothesis; no refinement (the projection search and
 * RefinePoseWithMatches follow at :279-284).  Host pointers, synchronous, one launch for the batch; the result is identical from run
 * to run.  n_problems == 0 is valid; n > 2048 is SNK_ERR_INVALID_ARG. */
SNK_API int snk_sim3_ransac(snk_matcher* m, const snk_sim3_params* params, snk_sim3_problem* problems, int n_problems);

/* The same for ONE problem with every hypothesis laid open, for tests (LoopDetector.cpp:205 has no counterpart: the loop is inside
 * the solver): triplets[k] = the three pair indices of hypothesis k, valid[k] = the triplet gave a transform, T[k] / scale[k] /
 * counts[k] = that transform and its inlier count (zeros when not valid).  All arrays have K entries, K = params->iterations when
 * that is > 0, else snk_ransac_iterations(problem->n, ...).  `problem` is filled as by snk_sim3_ransac. */
SNK_API int snk_sim3_debug_hypotheses(snk_matcher* m, const snk_sim3_params* params, snk_sim3_problem* problem,
                                      int32_t (*triplets)[3], int32_t* valid, double (*T)[7], double* scale, int32_t* counts);

/* Device-resident form for a batch of keyframe pairs (b = 0 .. frames1->batch - 1; keyframe 1 = source, 2 = target) --
 * LoopDetector.cpp:163-198, 250-278 with Snake/LoopClosing/LoopORBMatcher.cpp:110-116: pairs_dev [batch][pairs_cap][2] = (f1, f2),
 * n_pairs_dev [batch] is the output of snk_bf_filter_batch_dev with keyframe 1 as the query set.  An entry becomes a pair when both
 * features carry a point, 0 <= frame_pt1_dev[b][f1] < n_pts1_dev[b] and 0 <= frame_pt2_dev[b][f2] < n_pts2_dev[b]; the pairs keep
 * the order of the entries.  points1 = poses1_dev[b] * (3 doubles at pts1_dev + (b * pts_cap + frame_pt1) * pts_stride), points2
 * likewise (:193-194, computed by the kernel), ips = frames1->kps[b][f1] / frames2->kps[b][f2]; problem index = b; with
 * params->iterations = 0 the count is looked up in a table of snk_ransac_iterations kept by the handle.  Out: T_dev [batch][7],
 * scale_dev [batch] and corrected_pose_dev [batch][7] = tmpPose of :251-255,278, (R^T R2, R^T (t2 - t) / scale) with (R2, t2) =
 * poses2_dev[b] -- all three untouched without a winner; inliers_dev [batch]; match12_dev [batch][frames1->cap] = the point index
 * of keyframe 2 at every inlier's f1 and -1 everywhere else (vpMapPointMatches of :265-269 as indices).  pairs_cap <= 2048.
 * Asynchronous on the handle's stream: kNN-2 -> filter -> this call run without a host round trip. */
SNK_API int snk_sim3_ransac_pairs_batch_dev(snk_matcher* m, const snk_frames_dev* frames1, const snk_frames_dev* frames2,
                                            const snk_camera* cam, const snk_sim3_params* params, const int32_t* pairs_dev,
                                            const int32_t* n_pairs_dev, int pairs_cap, const void* pts1_dev, const void* pts2_dev,
                                            int pts_stride, const int32_t* frame_pt1_dev, const int32_t* frame_pt2_dev,
                                            const int32_t* n_pts1_dev, const int32_t* n_pts2_dev, int pts_cap, const double* poses1_dev,
                                            const double* poses2_dev, double* T_dev, double* scale_dev, int32_t* inliers_dev,
                                            int32_t* match12_dev, double* corrected_pose_dev);

/* ------------------------------------------------------------------------------------------
 * Local bundle adjustment
 * ------------------------------------------------------------------------------------------ */

/* The members of Saiga::OptimizationOptions / BAOptions that Snake sets
 * (Snake/Optimizer/LocalBundleAdjustment.cpp:47-64): maxIterations = 3, maxIterativeIterations = 30,
 * iterativeTolerance = 1e-10, solverType = Iterative with buildExplizitSchur, huberMono / huberStereo
 * = reprojectionErrorThreshold{Mono,Stereo} * lbaErrorFactor (Snake/System/SnakeGlobal.h:145-150).
 * lambda_init: initial LM damping (0 = 1e-4). */
typedef struct snk_ba_options
{
    int32_t max_iterations;
    int32_t max_pcg_iterations;
    double pcg_tol;
    double huber_mono, huber_stereo;
    double lambda_init;
} snk_ba_options;

/* One Saiga::Scene as MakeLocalScene fills it (LocalBundleAdjustment.cpp:187-293), flattened:
 * images[i] = {se3 (world -> camera; quaternion x y z w, translation), constant};
 * worldPoints[j] = {p, constant}; one entry per StereoImagePoint = {image, wp, point (pixels),
 * depth (> 0 => stereo observation; u_r = u - bf/depth), weight}; intrinsics[0] = K; scene.bf. */
/* Saiga RelPoseConstraint as MakeLocalScene fills it when the IMU is enabled
 * (LocalBundleAdjustment.cpp:294-346): img1 / img2 = id_in_scene of two consecutive keyframes,
 * rel_pose = the pre-integrated relative pose, weight_rotation = gyro weight / dt,
 * weight_translation = acc weight / dt (0 for dt > 2 s).  [DEFINED] (the residual lives in the absent
 * saiga): rel_pose is T_img2 * T_img1^-1 for world -> camera poses; e = log(T2 T1^-1 rel^-1) = (rho,
 * omega); r = (weight_translation * rho, weight_rotation * omega); cost += |r|^2 (no robust kernel);
 * Gauss-Newton Jacobians with J_l^-1 ~ I: d r / d delta2 = W, d r / d delta1 = -W Ad(T2 T1^-1). */
typedef struct snk_ba_rpc
{
    int32_t img1, img2;
    double rel_pose[7];
    double weight_rotation, weight_translation;
} snk_ba_rpc;

typedef struct snk_ba_problem
{
    int32_t n_img, n_pt, n_obs;
    double (*pose)[7];
    const uint8_t* img_const;
    double (*pt)[3];
    const uint8_t* pt_const;
    const int32_t* obs_img;
    const int32_t* obs_pt;
    const double (*obs_uv)[2];
    const double* obs_depth;
    const double* obs_weight;
    double K[4]; /* fx fy cx cy */
    double bf;
    int32_t n_rpc; /* scene.rel_pose_constraints (0 without IMU) */
    int32_t pad;
    const snk_ba_rpc* rpc;
} snk_ba_problem;

typedef struct snk_ba snk_ba;

SNK_API int snk_ba_create(const snk_ba_options* options, int device, void* stream, snk_ba** out);
SNK_API int snk_ba_destroy(snk_ba* h);
SNK_API int snk_ba_sync(snk_ba* h);

/* Replaces BARecRel::create(scene) — LocalBundleAdjustment.cpp:359: analyse the structure, copy
 * the problem to the device.  set_problems loads `count` independent windows that are solved side
 * by side (one launch sequence for all).  The arrays are copied; they need not stay alive.
 * Limits: count <= 65535; n_img <= 32767 per problem (SNK_ERR_INVALID_ARG beyond).
 * A call that returns anything but SNK_OK leaves the handle with NO problem set: the previous one
 * is gone as well (its device arrays may be partly overwritten), and solve, solve_async, reset,
 * get_state, residuals, set_outliers and solve_local_scene fail with "no problem set" until a
 * later set_problem(s) succeeds. */
SNK_API int snk_ba_set_problem(snk_ba* h, const snk_ba_problem* problem);
SNK_API int snk_ba_set_problems(snk_ba* h, const snk_ba_problem* problems, int count);

/* The same hand-over from DEVICE memory -- BARecRel::create (LocalBundleAdjustment.cpp:359) on the scenes a device-side MakeLocalScene
 * (LocalBundleAdjustment.cpp:94-346) left there: out_dev is the struct snk_scene_gather_batch_dev takes, a host struct of device pointers
 * (result [n_q] on the device too) with its four caps.  Problem s is row s with the sizes result[s].n_img / n_pt / n_obs / n_rpc, caller
 * order = the row's order; K and bf apply to every problem.  A row with status != SNK_SCENE_OK has all counts 0 and becomes an EMPTY
 * problem in slot s, so problem indices stay query indices -- and, like any problem without a free camera, an empty problem takes the
 * whole batch off the point-major pass: compact such rows away before the call where that matters.  rpc == NULL: no constraints.
 * obs_src, img_kf, pt_id and pt_valid are not read.  The values and the sorted observation arrays are written by kernels straight into
 * the handle's buffers; the host reads back about five bytes per observation of structure (free-camera indices, constant flags, point
 * starts, the constraint records) for the list stages that still run there, where snk_ba_set_problems carries 40 and more up.  A batch
 * with a problem of more than 8192 points, or with a point that holds more than 1024 valid observations, is staged instead: its rows
 * are copied down and go through snk_ba_set_problems' own path; the result is the same.
 * ORDER: the rows must be complete on the BA handle's stream, or the caller has synchronised their producer; the call waits for the
 * handle's stream, not for any other.  The rest of the contract is snk_ba_set_problems': the arrays are copied and need not stay
 * alive, n_q <= 65535, the implicit form takes one problem, any failure leaves NO problem set; after success every other snk_ba_* entry
 * point behaves as after snk_ba_set_problems on the same data.  Everything is checked before a kernel reads a row: a NULL handle,
 * struct, K, result or row array other than rpc / obs_src / img_kf / pt_id / pt_valid, a cap outside [1, limit] (the limits of
 * snk_scene_gather), n_q outside 1..65535, and -- the n_q records are read first, one small copy and one wait -- a record with a
 * negative count or a count above its cap (n_rpc above win_cap): SNK_ERR_INVALID_ARG.  Nothing past a row's counts is read. */
SNK_API int snk_ba_set_problems_dev(snk_ba* h, int n_q, const snk_scene_out* out_dev, const double K[4], double bf);

/* Saiga's BAOptions::buildExplizitSchur: the reference's local BA asks for the explicit Schur complement
 * (Snake/Optimizer/LocalBundleAdjustment.cpp:59), its global BA leaves it unset (Snake/Optimizer/GlobalBundleAdjustment.cpp:32-43)
 * and gets the implicit form.  1 (the default): the reduced camera system S is formed as a dense n6 x n6 matrix.  0: S is never
 * formed; every PCG iteration computes S p = U p + (constraint cross terms) - W V^-1 W^T p from the per-observation W blocks, so device
 * memory grows with the observations instead of the square of the free keyframes (global BA on maps of thousands of keyframes).
 * Takes effect at the next snk_ba_set_problem(s); in implicit mode set_problems with count > 1 fails with SNK_ERR_INVALID_ARG (a
 * global BA is one scene) and leaves no problem set.  Any value but 0 or 1: SNK_ERR_INVALID_ARG, the handle is unchanged. */
SNK_API int snk_ba_set_explicit_schur(snk_ba* h, int explicit_schur);

/* Which form of the reduced-camera-system PCG the last successful set_problem(s) chose (read-only;
 * tests and diagnostics).  *workgroups: the workgroups of the one-launch forms, 0 for the others.
 * A refused cooperative launch during a solve turns the handle to SNK_BA_PCG_LAUNCHES. */
enum
{
    SNK_BA_PCG_PER_PROBLEM  = 0, /* one workgroup per problem (S fits one workgroup's LDS) */
    SNK_BA_PCG_LAUNCHES     = 1, /* multi-launch pcgl_* sequence (vectors in HBM) */
    SNK_BA_PCG_PERSIST      = 2, /* one cooperative launch, two grid barriers per iteration */
    SNK_BA_PCG_PERSIST1     = 3, /* one cooperative launch, one grid barrier, rows of S streamed */
    SNK_BA_PCG_PERSIST_REG  = 4, /* one cooperative launch, one grid barrier, rows of S in registers */
    SNK_BA_PCG_IMPLICIT     = 5, /* implicit Schur form (snk_ba_set_explicit_schur(h, 0)): one cooperative launch */
    SNK_BA_PCG_IMPLICIT_LAUNCHES = 6  /* implicit Schur form, multi-launch (refused cooperative launch, recorded graphs) */
};
SNK_API int snk_ba_pcg_form(const snk_ba* h, int* form, int* workgroups);

/* Observations flagged here are ignored by solve / residuals, like StereoImagePoint::outlier
 * (LocalBundleAdjustment.cpp:382,391).  obs_outlier has n_obs entries in caller order; NULL clears. */
SNK_API int snk_ba_set_outliers(snk_ba* h, int problem, const uint8_t* obs_outlier);

/* Replaces BARecRel::initAndSolve() / solve() — LocalBundleAdjustment.cpp:365,407: `iterations`
 * LM iterations on every loaded problem (state stays on the device; fetch it with
 * snk_ba_get_state).  cost_initial / cost_final (one per problem, may be NULL) mirror
 * OptimizationResults::cost_initial / cost_final (LocalBundleAdjustment.cpp:412). */
SNK_API int snk_ba_solve(snk_ba* h, int iterations, double* cost_initial, double* cost_final);
SNK_API int snk_ba_solve_async(snk_ba* h, int iterations); /* enqueue only */
SNK_API int snk_ba_reset(snk_ba* h);                       /* restore the poses / points given to set_problems */

/* Optimised scene.images[i].se3 / scene.worldPoints[j].p (LocalBundleAdjustment.cpp:485-498). */
SNK_API int snk_ba_get_state(snk_ba* h, int problem, double (*pose)[7], double (*pt)[3], int* pcg_iterations);

/* Replaces the per-observation Scene::residual3 / residual2 squared norms of the chi-square outlier
 * passes (LocalBundleAdjustment.cpp:372-395, 423-457): chi2_per_obs[o] = |weighted residual|^2 at the
 * current state (0 for skipped observations), n_obs entries in caller order. */
SNK_API int snk_ba_residuals(snk_ba* h, int problem, double* chi2_per_obs);

/* LocalBundleAdjustment::SolveLocalScene after scene creation in ONE call (LocalBundleAdjustment.cpp:357-410): initAndSolve with
 * the handle's max_iterations (:357-365), the chi-square pass on the device (:368-397: every observation that is valid, not
 * yet an outlier and has chi2 > (depth > 0 ? chi2_stereo : chi2_mono) becomes an outlier), `extra_iterations` more iterations
 * when anything was marked (:399-410; the reference uses 1).  One 4-byte count crosses the bus in between instead of the chi2
 * array down and the mask up.  Results: *n_marked (outlierPoints), the FIRST solve's costs (what :412 returns), the optimised
 * poses / points of `problem` and its observation outlier flags after the pass (n_obs bytes, caller order); each may be NULL
 * except n_marked.  Same results as snk_ba_solve -> snk_ba_residuals -> host threshold -> snk_ba_set_outliers -> snk_ba_solve.
 * With several problems loaded every problem is solved and marked, and each one that had something marked gets the extra
 * iterations (decided on the device: the call synchronises once, at the end); the outputs are those of `problem`. */
SNK_API int snk_ba_solve_local_scene(snk_ba* h, int problem, double chi2_mono, double chi2_stereo, int extra_iterations,
                                     uint8_t* obs_outlier, int* n_marked, double* cost_initial, double* cost_final,
                                     double (*pose)[7], double (*pt)[3]);

/* ------------------------------------------------------------------------------------------
 * Pose-graph optimisation of the loop corrector -- semantics "snk-pgo v1" 
 * ------------------------------------------------------------------------------------------
 * Replaces: the solve behind LoopClosing::OptimizeEssentialGraph (Snake/LoopClosing/LoopClosingPGO.cpp:120-264: PGORec / PGOSim3Rec
 * create + initAndSolve at :134-146, the map-point pass at :231-260) on the graph LoopClosing::ConstructPGO leaves
 * (LoopClosingPGO.cpp:16-118).  saiga's solver is absent: the residual, the update, the exact Jacobians, the LM schedule and the
 * linear solve are [DEFINED] in DESIGN.md section 3f and restated in tests/pgo_numpy.py.
 * A pose is 8 doubles qx qy qz qw tx ty tz s (T_w_i, x -> s R x + t); s is read only when fix_scale == 0.
 * Limits: up to SNK_PGO_MAX_VERTICES vertices and SNK_PGO_MAX_EDGES edges.  Graphs whose rows do not fit the resident PCG kernel
 * (more workgroups than the device holds at once, or one vertex with more than about 380 free neighbours) are solved by the
 * multi-launch PCG instead of being refused.  One handle per thread; calls on a handle are serial and synchronous. */
typedef struct snk_pgo snk_pgo;
#define SNK_PGO_MAX_VERTICES 10000 /* the keyframe limit of snk_ba */
#define SNK_PGO_MAX_EDGES 200000   /* 1 304 bytes of device memory per edge: 260 MB */

typedef struct snk_pgo_options
{
    int32_t max_iterations;     /* LM iterations, 50 at LoopClosingPGO.cpp:125 */
    int32_t max_pcg_iterations; /* cap of the PCG per LM iteration; 10000 (the most a test graph takes is 2 078) */
    double pcg_tol;             /* stop when r.z <= pcg_tol * (r.z at the start); 1e-20, i.e. 1e-10 on the preconditioned residual norm */
    double min_chi2_delta;      /* stop after the first accepted step that lowers the cost by less; 1e-10 at LoopClosingPGO.cpp:126 */
    double lambda_init;         /* 1e-4, the schedule of snk-ba v1 */
} snk_pgo_options;

typedef struct snk_pgo_result
{
    double cost_initial, cost_final; /* what LoopClosingPGO.cpp:137-139 prints */
    int32_t lm_iterations, pcg_iterations_total, accepted_steps;
    int32_t pcg_form;   /* of the last linear solve: 0 none ran, 1 one cooperative launch (resident), 2 one launch per phase */
    int32_t workgroups; /* of that solve */
    int32_t pcg_iterations_max; /* the most PCG iterations one linear solve took: equal to max_pcg_iterations when the cap cut a solve short */
} snk_pgo_result;

SNK_API int snk_pgo_create(const snk_pgo_options* options, int device, void* stream, snk_pgo** out);
SNK_API int snk_pgo_destroy(snk_pgo* h);
/* The result of ConstructPGO (LoopClosingPGO.cpp:16-118): vertices with their constant flags (:63-70), edges (i, j) with i < j, unique
 * and sorted (:90,99,108), weights (NULL: all 1).  measurements[e] = T_i_j; NULL: T_w_i^-1 T_w_j of poses_measure, the poses the edges
 * are measured at (AddVertexEdge at :105, before SetPose at :114 moves the corrected vertices).  poses_init: the start state (NULL:
 * poses_measure).  Refused with SNK_ERR_INVALID_ARG and a text in snk_last_error(): i >= j, duplicate or unsorted edges, indices out of
 * range, non-finite input, with fix_scale a scale other than 1 (without: a scale <= 0).  Zero vertices or zero edges is valid.  A refused
 * call changes nothing: the handle stays usable and keeps the graph it had. */
SNK_API int snk_pgo_set_graph(snk_pgo* h, int n_vertices, const double (*poses_measure)[8], const double (*poses_init)[8],
                              const uint8_t* constant, int n_edges, const int32_t (*edges)[2], const double* weights,
                              const double (*measurements)[8], int fix_scale);
/* initAndSolve (LoopClosingPGO.cpp:134-146). */
SNK_API int snk_pgo_solve(snk_pgo* h, snk_pgo_result* result);
/* The current state (LoopClosingPGO.cpp:148-229 read the optimised vertices back). */
SNK_API int snk_pgo_get_poses(snk_pgo* h, double (*poses)[8]);
/* sum of |r_e|^2 at the current state (the chi2 of LoopClosingPGO.cpp:137-139). */
SNK_API int snk_pgo_cost(snk_pgo* h, double* cost);
/* Tests: linearises at the current state; residuals [E][7], gradient J^T r [n][7] and diagonal blocks [n][49] of ALL vertices (constant
 * ones included, before damping); the se3 form leaves entry / row / column 6 zero.  Each may be NULL. */
SNK_API int snk_pgo_debug_linearisation(snk_pgo* h, double (*residuals)[7], double (*gradient)[7], double (*diag)[49]);
/* The map-point pass of OptimizeEssentialGraph (LoopClosingPGO.cpp:231-247; MapPoint::Transform spelled out at :256-260): point k with
 * reference vertex ref_vertex[k] moves by T_w_i^after (T_w_i^before)^-1 as a Sim3 -- position, normal (rotation only), reference_depth
 * times the scale -- where before = poses_measure of the last snk_pgo_set_graph and after = the current state.  ref -1 or a constant
 * vertex: untouched.  Host pointers; normals and reference_depth may be NULL. */
SNK_API int snk_pgo_transform_points(snk_pgo* h, int n_points, const int32_t* ref_vertex, double (*positions)[3], double (*normals)[3],
                                     double* reference_depth);

/* ------------------------------------------------------------------------------------------
 * Bag-of-words place recognition -- semantics "snk-bow v1" 
 * ------------------------------------------------------------------------------------------
 * Replaces, in the order the loop closer and the relocaliser run them: `vocabulary.transform(descriptors, bow_vec, bow_feature_vec, 4,
 * threads)` of Frame::computeBoW (Snake/Map/Frame.cpp:38-40), KeyframeDatabase::Add / Remove / DetectLoopCandidates /
 * DetectRelocalizationCandidates (Snake/LoopClosing/KeyframeDatabase.cpp:20-168; call sites Snake/LoopClosing/LoopDetector.cpp:69-87 and
 * Snake/Tracking/TrackingCoarse.cpp:521), `vocabulary.score` (LoopDetector.cpp:73) and LoopORBmatcher::MatchBoW
 * (Snake/LoopClosing/LoopORBMatcher.cpp:121-215, called at LoopDetector.cpp:225).  Saiga::MiniBow2 and ORBvoc.minibow are absent: the
 * descent, the weighting and the score are [DEFINED] in DESIGN.md section 3g (DBoW2's published rules) and restated in
 * tests/bow_numpy.py; parity with MiniBow2 itself is not pinned.
 * Limits: SNK_BOW_MAX_FEATURES features per frame (and words per query or database row), SNK_BOW_MAX_CANDIDATES candidates per query,
 * a vocabulary of depth <= SNK_BOW_MAX_DEPTH.  One handle per thread; a database works on its vocabulary's stream. */
typedef struct snk_bow_vocab snk_bow_vocab;
typedef struct snk_bow_db snk_bow_db;
#define SNK_BOW_MAX_FEATURES 2048
#define SNK_BOW_MAX_CANDIDATES 64
#define SNK_BOW_MAX_DEPTH 16

/* The vocabulary `ORBVocabulary vocabulary` of Snake/System/System.cpp:44 as a rooted tree in flat arrays: node 0 is the root; node i
 * has the children children[child_start[i] .. child_start[i] + child_count[i]) (child_count 0 = leaf), the descriptor desc[i] (the
 * root's is unused), word_id[i] (dense 0 .. n_words - 1 on leaves, -1 inside) and weight[i] (leaves).  The tree may be irregular.
 * Validated on the host before a device is touched: every non-root node the child of exactly one node, no cycle, every leaf a word id
 * and each id once, depth <= 16, weights finite and >= 0 -- anything else is SNK_ERR_INVALID_ARG with the reason in snk_last_error(). */
SNK_API int snk_bow_vocab_create(int n_nodes, const int32_t* child_start, const int32_t* child_count, const int32_t* children,
                                 int n_children, const uint64_t (*desc)[4], const int32_t* word_id, const double* weight, int device,
                                 void* stream, snk_bow_vocab** out);
SNK_API int snk_bow_vocab_destroy(snk_bow_vocab* v);
/* vocabulary.size() (KeyframeDatabase.cpp:15-16) = *n_words; also the node count and the depth L of the deepest leaf.  Each may be NULL. */
SNK_API int snk_bow_vocab_size(const snk_bow_vocab* v, int* n_words, int* n_nodes, int* depth);

/* Frame::computeBoW (Frame.cpp:38-40) for one frame in host memory, n <= SNK_BOW_MAX_FEATURES.  bow_vec: words[*n_words] ascending with
 * values (count * weight, divided by the L1 norm; *n_words = 0 when the norm is 0).  bow_feature_vec in the snk_bow_features layout:
 * node_id[*n_nodes] strictly ascending, node_start[*n_nodes + 1], features ascending inside a node; the node of a feature is the one on
 * its path at depth L - levelsup, and a feature whose node would be the root (L - levelsup <= 0, or a leaf above that depth) is in no
 * node.  word_of_feature[n] / node_of_feature[n] (0 = none).  Arrays hold n entries, node_start n + 1. */
SNK_API int snk_bow_transform(snk_bow_vocab* v, const uint64_t (*desc)[4], int n, int levelsup, int32_t* words, double* values,
                              int* n_words, uint32_t* node_id, int32_t* node_start, int32_t* features, int* n_nodes,
                              int32_t* word_of_feature, int32_t* node_of_feature);
/* The same for every frame of a batch that lies in HBM (frames->desc [batch][cap][4], frames->n [batch]; the other members are not
 * read): straight behind snk_orb_detect_batch_dev / snk_feature_grid_batch_dev.  Outputs [batch][cap], node_start [batch][cap + 1],
 * n_words / n_nodes [batch]; word_of_feature is -1 and node_of_feature 0 behind a frame's n.  cap <= SNK_BOW_MAX_FEATURES.
 * Asynchronous on the vocabulary's stream (Frame.cpp:38-40). */
SNK_API int snk_bow_transform_batch_dev(snk_bow_vocab* v, const snk_frames_dev* frames, int levelsup, int32_t* words_dev,
                                        double* values_dev, int32_t* n_words_dev, uint32_t* node_id_dev, int32_t* node_start_dev,
                                        int32_t* features_dev, int32_t* n_nodes_dev, int32_t* word_of_feature_dev,
                                        int32_t* node_of_feature_dev);
/* `vocabulary.score(a, b)` (LoopDetector.cpp:73): the L1 score -1/2 sum over the common words of (|a_w - b_w| - a_w - b_w), in double.
 * Both vectors are in host memory, so this is a merge on the host; the database entry points below score on the device. */
SNK_API int snk_bow_score(const snk_bow_vocab* v, const int32_t* words_a, const double* values_a, int n_a, const int32_t* words_b,
                          const double* values_b, int n_b, double* score);

/* KeyframeDatabase (KeyframeDatabase.cpp:10-18): device-resident, one row of at most max_words <= SNK_BOW_MAX_FEATURES words per
 * keyframe, no inverted file. */
SNK_API int snk_bow_db_create(snk_bow_vocab* v, int max_keyframes, int max_words, snk_bow_db** out);
SNK_API int snk_bow_db_destroy(snk_bow_db* db);
/* KeyframeDatabase::Add (KeyframeDatabase.cpp:20-26).  An id that is already stored, a negative id, unsorted words or a full database:
 * SNK_ERR_INVALID_ARG, nothing changes. */
SNK_API int snk_bow_db_add(snk_bow_db* db, int kf_id, const int32_t* words, const double* values, int n);
/* Add for `count` keyframes whose rows the batched transform left in HBM: kf_ids [count] on the host, words_dev / values_dev
 * [count][cap], n_words_dev [count], cap <= max_words is not required (a longer row is cut at max_words) (KeyframeDatabase.cpp:20-26). */
SNK_API int snk_bow_db_add_batch_dev(snk_bow_db* db, const int32_t* kf_ids, int count, const int32_t* words_dev,
                                     const double* values_dev, const int32_t* n_words_dev, int cap);
/* KeyframeDatabase::Remove (KeyframeDatabase.cpp:28-56).  An id that is not stored: SNK_ERR_INVALID_ARG.  The id may be added again. */
SNK_API int snk_bow_db_remove(snk_bow_db* db, int kf_id);
/* GetKeyframesWithSharingWords + RemoveWeakMatches (KeyframeDatabase.cpp:100-168) as DetectLoopCandidates (:58-80: exclude_ids = the
 * connected keyframes, 0.8, 0.75, minScore) and DetectRelocalizationCandidates (:83-98: no exclusion, 0.8, 0.75, 0) call them: the
 * stored keyframes with >= 1 common word that are not excluded; drop common < sharing_word_ratio * maxCommon (float, :137); score;
 * drop score < score_ratio * best or < min_score (double); order by score descending, ties to the lower id; the first
 * max_candidates <= SNK_BOW_MAX_CANDIDATES.  out_ids / out_scores / out_common hold max_candidates entries (out_common may be NULL). */
SNK_API int snk_bow_db_query(snk_bow_db* db, const int32_t* words, const double* values, int n, const int32_t* exclude_ids,
                             int n_exclude, float sharing_word_ratio, float score_ratio, float min_score, int max_candidates,
                             int32_t* out_ids, double* out_scores, int32_t* out_common, int* n_out);
/* n_queries queries in one launch pair (relocalising many frames, TrackingCoarse.cpp:521, or checking many keyframes,
 * LoopDetector.cpp:69-87): words_dev / values_dev [n_queries][cap], n_words_dev [n_queries]; exclude_ids_dev [n_queries][exclude_cap]
 * with n_exclude_dev [n_queries], or NULL; outputs [n_queries][max_candidates] and n_out_dev [n_queries].  Asynchronous. */
SNK_API int snk_bow_db_query_batch_dev(snk_bow_db* db, int n_queries, const int32_t* words_dev, const double* values_dev,
                                       const int32_t* n_words_dev, int cap, const int32_t* exclude_ids_dev, const int32_t* n_exclude_dev,
                                       int exclude_cap, float sharing_word_ratio, float score_ratio, float min_score, int max_candidates,
                                       int32_t* out_ids_dev, double* out_scores_dev, int32_t* out_common_dev, int32_t* n_out_dev);

/* Replaces LoopORBmatcher::MatchBoW(source, target, matches, 50, 0.75) -- LoopORBMatcher.cpp:121-215, call site LoopDetector.cpp:225.
 * desc / has_mp (GetMapPoint(i) != nullptr and not bad) of each keyframe, bow = its bow_feature_vec.  match12[n1] = the feature of
 * keyframe 2 whose map point vpMatches12 would hold, or -1; *n_matches = the return value.  0 <= threshold <= 256. */
SNK_API int snk_match_loop_bow(snk_matcher* m, const uint64_t (*desc1)[4], const uint8_t* has_mp1, int n1, const snk_bow_features* bow1,
                               const uint64_t (*desc2)[4], const uint8_t* has_mp2, int n2, const snk_bow_features* bow2, int threshold,
                               float ratio, int32_t* match12, int* n_matches);
/* MatchBoW (LoopORBMatcher.cpp:121-215) for every keyframe pair of a batch in HBM: frames (desc, n), has_mp [batch][cap] and the
 * feature vectors as snk_bow_transform_batch_dev leaves them.  match12_dev [batch][frames1->cap]; pairs_dev [batch][frames1->cap][2] =
 * (feature of keyframe 1, feature of keyframe 2) ascending in the first, n_pairs_dev [batch]: the layout
 * snk_sim3_ransac_pairs_batch_dev takes, with pairs_cap = frames1->cap.  Asynchronous on the matcher's stream. */
SNK_API int snk_match_loop_bow_batch_dev(snk_matcher* m, const snk_frames_dev* frames1, const snk_frames_dev* frames2,
                                         const uint8_t* has_mp1_dev, const uint8_t* has_mp2_dev, const uint32_t* node_id1_dev,
                                         const int32_t* node_start1_dev, const int32_t* features1_dev, const int32_t* n_nodes1_dev,
                                         const uint32_t* node_id2_dev, const int32_t* node_start2_dev, const int32_t* features2_dev,
                                         const int32_t* n_nodes2_dev, int threshold, float ratio, int32_t* match12_dev,
                                         int32_t* pairs_dev, int32_t* n_pairs_dev);

/* ------------------------------------------------------------------------------------------
 * Keyframe culling (snk-simp v1)
 * ------------------------------------------------------------------------------------------
 * Simplification::KeyFrameCullingGraph and Redundancy (Snake/Optimizer/Simplification.cpp:148-358, :75-146), Keyframe::MatchCount and
 * ComputeDepthRange (Snake/Map/Keyframe.cpp:68-77, :175-206) for many keyframes per call, in two stages: per-keyframe statistics from
 * the map tables, then the decision from the connection lists.  saiga's WeightedUndirectedGraph is not part of the reference checkout:
 * the graph rules (edge weight, spanning tree, weakest link) are [DEFINED] in DESIGN.md section 3l and restated in tests/simp_numpy.py.
 * Every query of a call sees the same tables.  EraseKeyframe (:55), the re-queue of the three best covisible keyframes (:50-63: the last
 * three entries of q's list), UpdateConnections of :207 and the choice of how many verdicts of one call to apply stay with the caller. */

#define SNK_SIMP_MAX_NODES 256  /* q and its connections of weight >= min_matches_in_graph; node_cap at most */
#define SNK_SIMP_MAX_FEAT 16384 /* feat_cap at most: a float per feature of the query in LDS */

#define SNK_SIMP_OK 0
#define SNK_SIMP_SKIPPED 1        /* the query keyframe is bad (Simplification.cpp:93, :217) */
#define SNK_SIMP_FEAT_OVERFLOW 2  /* the query has more than feat_cap features */
#define SNK_SIMP_NODES_OVERFLOW 3 /* more than node_cap nodes: no decision */
#define SNK_SIMP_BAD_INDEX 4      /* device forms: an id, a start or a feature index outside its range */

#define SNK_SIMP_NONE 0 /* no decision (status != SNK_SIMP_OK) */
#define SNK_SIMP_FACTOR 1
#define SNK_SIMP_NO_CONN 2
#define SNK_SIMP_ANGLE 3
#define SNK_SIMP_MATCHES 4
#define SNK_SIMP_REDUNDANCY 5
#define SNK_SIMP_LINK 6 /* reasons 1 .. 6 cull */
#define SNK_SIMP_KEEP_IMU_WEIGHTS 7
#define SNK_SIMP_KEEP_TIME_GAP 8
#define SNK_SIMP_KEEP_BRANCH 9
#define SNK_SIMP_KEEP_DISCONNECTED 10
#define SNK_SIMP_KEEP_LINK 11

/* The map as tables: the layouts and names of snk_covis_map / snk_scene_map.  Host pointers for snk_simp_stats, device pointers for the
 * _batch_dev form. */
typedef struct snk_simp_map
{
    int32_t n_kf, n_points, n_obs, n_feat;
    const uint8_t* kf_bad;      /* [n_kf] */
    const double* kf_pose;      /* [n_kf][7] world -> camera: qx qy qz qw tx ty tz */
    const int32_t* feat_start;  /* [n_kf + 1], feat_start[0] = 0 */
    const int32_t* feat_point;  /* [n_feat] point ids, -1: none */
    const float* feat_depth;    /* [n_feat] frame->depth[i] */
    const int32_t* feat_octave; /* [n_feat] undistorted_keypoints[i].octave */
    const int32_t* obs_start;   /* [n_points + 1], obs_start[0] = 0 */
    const int32_t (*obs)[2];    /* [n_obs] GetObservationList() in list order as (kf, feature index inside the keyframe) */
    const uint8_t* pt_flags;    /* [n_points] SNK_COVIS_PT_BAD; the other bits are not read */
    const double* pt_pos;       /* [n_points][3] */
} snk_simp_map;

typedef struct snk_simp_stats_params
{
    int32_t min_obs;  /* MatchCount's argument; Simplification.cpp:282 passes 3 */
    int32_t stereo;   /* settings.inputType != Mono (:107): features deeper than th_depth do not enter the redundancy */
    float th_depth;   /* :109; equality counts */
    int32_t feat_cap; /* features of one query at most, 1 .. SNK_SIMP_MAX_FEAT */
} snk_simp_stats_params;

/* One query of stage 1.  status != SNK_SIMP_OK: median_depth = -1, the counts and the redundancy 0. */
typedef struct snk_simp_stats_result
{
    float median_depth;  /* ComputeDepthRange(true); -1 (the member's initial value, Keyframe.h:125) where n_depth == 0 */
    int32_t n_depth;     /* features with a point, bad points included (Keyframe.cpp:189) */
    int32_t match_count; /* MatchCount(min_obs) */
    int32_t n_mps;       /* nMPs of Redundancy */
    int32_t n_redundant; /* nRedundantObservations */
    float redundancy;    /* (float)n_redundant / (float)n_mps; 0 / 0 is NaN and compares false, as in the reference */
    int32_t status;
} snk_simp_stats_result;

/* Stage 1 for the keyframes q[0 .. n_q).  ComputeDepthRange(always = true) — Snake/Map/Keyframe.cpp:183-205: for every feature of q with
 * a point (bad ones too) z = (float)(row 3 of R(q) . p + t_z) in double, in the operation order simp_core.hpp states; median_depth is
 * the element (n_depth - 1) / 2 of the ascending order, [DEFINED] the total order of the IEEE bit patterns (-0 before +0; the inputs are
 * finite).  MatchCount(min_obs) — Keyframe.cpp:68-77: the features whose point is not bad and has at least min_obs observations,
 * [DEFINED] GetNumObservations() = obs_start[p + 1] - obs_start[p].  Redundancy — Simplification.cpp:98-145: over the features with a
 * point that is not bad (stereo: feat_depth <= th_depth only) n_mps += 1; a list longer than 3 is walked in order, entries of q itself
 * skipped, those with feat_octave[feat_start[k] + f] <= the feature's octave + 1 counted; 3 or more: n_redundant += 1.  Bad observer
 * keyframes count.  q bad (:93): SNK_SIMP_SKIPPED.  The caller leaves its cached median alone where n_depth == 0 (Keyframe.cpp:199-202).
 * Everything is checked before anything is launched: a NULL array with a non-zero count, starts that do not begin at 0 or decrease, a
 * query, a point id, an observation's keyframe or feature index outside its range, n_kf > SNK_COVIS_MAX_KF, feat_cap outside
 * [1, SNK_SIMP_MAX_FEAT]: SNK_ERR_INVALID_ARG.  n_q == 0 is valid.  The results do not depend on the kernel form
 * (SNK_SIMP_LONG_MIN=<n> moves the length from which a wavefront walks a list, read once). */
SNK_API int snk_simp_stats(snk_matcher* m, const snk_simp_map* map, const snk_simp_stats_params* params, int n_q, const int32_t* q,
                           snk_simp_stats_result* out);

/* The same (Keyframe.cpp:68-77, :183-205, Simplification.cpp:98-145) with every table, q_dev and out_dev on the device.  Asynchronous on
 * the handle's stream, no host round trip.  The scalars are checked on the host; the kernel checks what the host cannot see, as
 * snk_covis_update_batch_dev does -- a query outside [0, n_kf), a feature range outside [0, n_feat] or decreasing, a point id outside
 * [-1, n_points), an obs_start outside [0, n_obs] or decreasing, an observation's keyframe outside [0, n_kf) -- and an observation's
 * feature index outside its keyframe's range: that query has status = SNK_SIMP_BAD_INDEX, nothing outside the ranges is read, the
 * other queries are unaffected.  Only the lists a query walks are checked. */
SNK_API int snk_simp_stats_batch_dev(snk_matcher* m, const snk_simp_map* map_dev, const snk_simp_stats_params* params, int n_q,
                                     const int32_t* q_dev, snk_simp_stats_result* out_dev);

/* The keyframe side of the decision.  Host pointers for snk_simp_decide, device pointers for the _batch_dev form.  kf_prev, kf_next and
 * kf_time are all NULL or all present. */
typedef struct snk_simp_graph
{
    int32_t n_kf, n_list;
    const uint8_t* kf_bad;                  /* [n_kf] */
    const double* kf_pose;                  /* [n_kf][7] */
    const float* kf_cull_factor;            /* [n_kf] kf->cull_factor */
    const double* kf_median_depth;          /* [n_kf] the cached member: the caller fills the entries <= 0 from stage 1 before the call (the
                                               lazy rule of Keyframe.cpp:177); read as it is, -1 included */
    const int32_t* kf_prev;                 /* [n_kf] previousKF as a slot, -1: none */
    const int32_t* kf_next;                 /* [n_kf] nextKF */
    const double* kf_time;                  /* [n_kf] frame->timeStamp */
    const int32_t* conn_start;              /* [n_kf + 1] */
    const struct snk_covis_conn* conn_list; /* [n_list] every keyframe's connections ascending by (weight, kf): the arguments of
                                               snk_scene_window / snk_lmap_select, as snk_covis_update leaves them */
} snk_simp_graph;

typedef struct snk_simp_params
{
    int32_t min_matches_in_graph; /* simpl_min_matches_in_graph: 20 */
    float border_angle;           /* simpl_border_angle: 1.0 */
    float border_redundancy;      /* simpl_border_redundancy: 0.8 */
    int32_t border_matches;       /* simpl_border_matches: 80 */
    int32_t th_map;               /* settings.th_map: 140 */
    int32_t with_imu;             /* WITH_IMU (Simplification.cpp:158) */
    double gyro_weight;           /* current_gyro_weight */
    double acc_weight;            /* current_acc_weight */
    float max_time_between_kf;    /* max_time_between_kf_map: 0.5 */
} snk_simp_params;

/* One query of stage 2.  status != SNK_SIMP_OK: reason = SNK_SIMP_NONE, everything else 0. */
typedef struct snk_simp_verdict
{
    int32_t reason;       /* SNK_SIMP_FACTOR .. SNK_SIMP_KEEP_LINK */
    int32_t cull;         /* 1 exactly for FACTOR, NO_CONN, ANGLE, MATCHES, REDUNDANCY, LINK */
    double value;         /* the third element of the reference's tuple: the angle, the match count, the redundancy, the weakest link; else 0 */
    int32_t n_nodes;      /* nodes of the first graph, q included; 0 where a verdict fell before the graph */
    int32_t n_root_edges; /* tree edges at q */
    int32_t weakest_link; /* of the second tree, where it is connected; else 0 */
    int32_t status;
} snk_simp_verdict;

/* Stage 2 for the keyframes q[0 .. n_q) — Simplification::KeyFrameCullingGraph, Simplification.cpp:148-358 — in the reference's order.
 * stats [n_q] are the same queries' records of stage 1 with min_obs = 3; a status there other than OK is passed through.
 * q bad (:217): SNK_SIMP_SKIPPED.  cull_factor > 3 (:150): FACTOR.  with_imu (:158-179): a weight == 0 keeps (KEEP_IMU_WEIGHTS); with the
 * time tables, prev >= 0, next >= 0 and time[next] - time[prev] > max_time_between_kf keeps (KEEP_TIME_GAP).  Nodes (:222-239): id 0 is
 * q, then q's connections with weight >= min_matches_in_graph in list order, bad targets kept; a keyframe listed twice answers to its
 * last id, as the reference's id_map does; more than node_cap nodes: SNK_SIMP_NODES_OVERFLOW.  Edges (:242-246): q's filtered list, then
 * every node's full list, each entry whose target is a node; [DEFINED] undirected, a pair listed more than once has the maximum of its
 * weights, self edges are dropped.  BuildMST [DEFINED]: the MAXIMUM spanning tree by Prim from id 0 (:351 accepts culling where the
 * weakest link is large); an outside node keeps its best (weight, parent), the smaller parent among equal weights; the node with the
 * largest weight joins, the smallest id among equals; unreachable nodes stay outside.  No tree edge at id 0 (:256): NO_CONN.  One, to o
 * (:287-310): angle = atan2(0.5 |C_q - C_o|, (median[q] + median[o]) * 0.5) * 2 * (180 / pi); angle < border_angle * cull_factor: ANGLE;
 * else match_count < border_matches * cull_factor: MATCHES; else redundancy > border_redundancy: REDUNDANCY; else KEEP_BRANCH.  Two or
 * more (:316-357): the maximum tree of the graph on q's tree neighbours alone; a neighbour left outside (:342): KEEP_DISCONNECTED; its
 * smallest edge * cull_factor > th_map: LINK; else KEEP_LINK.  node_cap (1 .. SNK_SIMP_MAX_NODES) sizes the kernel's LDS: small
 * graphs pack many workgroups per compute unit.  Everything is checked before anything is launched: a NULL array with a non-zero count,
 * conn_start not beginning at 0 or decreasing, a query, a connection, kf_prev or kf_next outside its range, n_kf > SNK_COVIS_MAX_KF,
 * node_cap outside its range, time tables only partly present: SNK_ERR_INVALID_ARG.  n_q == 0 is valid. */
SNK_API int snk_simp_decide(snk_matcher* m, const snk_simp_graph* graph, const snk_simp_params* params, int node_cap, int n_q,
                            const int32_t* q, const snk_simp_stats_result* stats, snk_simp_verdict* out);

/* The same (Simplification.cpp:148-358) with every table, q_dev, stats_dev and out_dev on the device.  Asynchronous, no host round trip.
 * The kernel checks: a query outside [0, n_kf), kf_prev / kf_next outside [-1, n_kf), a conn_start range outside [0, n_list] or
 * decreasing, a connection's keyframe outside [0, n_kf) give that query SNK_SIMP_BAD_INDEX; only the ranges a query reaches are checked. */
SNK_API int snk_simp_decide_batch_dev(snk_matcher* m, const snk_simp_graph* graph_dev, const snk_simp_params* params, int node_cap, int n_q,
                                      const int32_t* q_dev, const snk_simp_stats_result* stats_dev, snk_simp_verdict* out_dev);

/* ------------------------------------------------------------------------------------------
 * Multi-GPU result gather (BASELINE config 5: one sequence per GPU)
 * ------------------------------------------------------------------------------------------
 * The path shards over independent units -- one Snake-SLAM process and one sequence per GPU -- and exchanges nothing while it
 * runs.  When a rank is done it holds what the reference writes per run: the TUM trajectory (Snake/System/System.cpp:552-563,
 * "timestamp tx ty tz qx qy qz qw" per frame) and a few counters.  These entry points gather such fixed-size blocks across the
 * ranks with ONE RCCL all-gather over xGMI, without torch.distributed or MPI in the process.  RCCL is opened at run time (dlopen
 * by SONAME librccl.so.1; SNK_RCCL_LIB overrides): the library has no link-time dependency on it.
 * Replaces: nothing in the reference (it is a single-GPU program); serves the "RCCL/xGMI only for result gather" of north_star.
 * One handle per process / GPU; calls on a handle are serial. */
typedef struct snk_dist snk_dist;
#define SNK_DIST_ID_BYTES 128 /* = NCCL_UNIQUE_ID_BYTES */

/* Rank 0 creates the 128-byte communicator id and hands it to the other ranks by any means (environment, file, socket). */
SNK_API int snk_dist_get_unique_id(uint8_t id[SNK_DIST_ID_BYTES]);
/* Collective over all `world` ranks (ncclCommInitRank): rank r runs on HIP device `device`.  Returns when every rank has called. */
SNK_API int snk_dist_init(const uint8_t id[SNK_DIST_ID_BYTES], int rank, int world, int device, snk_dist** out);
/* The same with the id passed through a file all ranks can see: rank 0 removes whatever an earlier job left at `path`, writes
 * the id (atomically: `path`.tmp + rename), the others wait up to timeout_s seconds (<= 0: 60) for it.  Rank 0 removes the file
 * again in snk_dist_destroy and when its init fails.  Use a fresh path per job, or start rank 0 first: a rank that reads a
 * stale file before rank 0 has removed it joins a dead communicator. */
SNK_API int snk_dist_init_file(const char* path, int rank, int world, int device, double timeout_s, snk_dist** out);
SNK_API int snk_dist_destroy(snk_dist* d);
SNK_API int snk_dist_rank(const snk_dist* d, int* rank, int* world);
/* recv[r * bytes .. (r + 1) * bytes) = rank r's `send` block, on every rank; every rank passes the same `bytes`.  Host memory
 * (staged through one pinned buffer: upload, ncclAllGather on the handle's stream, download, one synchronisation). */
SNK_API int snk_dist_all_gather(snk_dist* d, const void* send, size_t bytes, void* recv);
/* Device memory, no staging; returns after the handle's stream has drained. */
SNK_API int snk_dist_all_gather_dev(snk_dist* d, const void* send_dev, size_t bytes, void* recv_dev);
/* Maximum of one value per rank on every rank (the longest trajectory: blocks are padded to it); doubles as a barrier. */
SNK_API int snk_dist_max_i64(snk_dist* d, int64_t value, int64_t* out);
/* ncclGetVersion of the RCCL this process resolved (SNK_ERR_NO_DEVICE when none can be opened). */
SNK_API int snk_dist_rccl_version(int* version);

#ifdef __cplusplus
}
#endif
#endif /* SNAKE_HIP_H */
