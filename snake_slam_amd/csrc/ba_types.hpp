// Bundle adjustment: what the solver (ba.hip: every LM / PCG kernel, the launch sequence, state and results) and the scene hand-over
// (ba_handover.hip: snk_ba_set_problems, which turns the caller's scenes into the device lists those kernels walk) share -- the
// records of the device lists, the kernel argument block, the handle, and the three functions one side calls on the other.
// Two translation units see these types, so they live in a named namespace (an anonymous one would give snk_ba a different member
// type in each).
#pragma once
#include "common.hpp"
#include "dispatch.hpp"

#include <algorithm>
#include <condition_variable>
#include <cstdlib>
#include <functional>
#include <map>
#include <mutex>
#include <thread>
#include <utility>
#include <vector>

namespace snk
{
namespace ba
{
struct Prob
{
    int ni, np, no;     // images, points, valid observations (sorted by point)
    int nfc, n6;        // free cameras, 6 * nfc
    int img_off, pt_off, obs_off, cam_off;
    int ptstart_off, camstart_off, citem_off, blkstart_off, ent_off;
    int vec_off;        // n6-vectors (rhs, x)
    long long s_off;    // S (n6 * n6 doubles)
    int orig_off;       // first caller-order observation of this problem
    int n_wv;           // wavefront work items of point_wave (whole points, <= 64 observations each); 0: not available
    int wv_off;
    int n_rpc;          // valid relative pose constraints (IMU scenes)
    int rpc_off;        // into rpc_meta / rpc_out
    int camrpc_off;     // into cam_rpc_start (nfc + 1 entries per problem)
    int n_set;          // work items of schur_set (0: not available for this problem)
    int set_off;        // into set_items
    int cblk_off;       // into cblk_start (nfc * nfc + 1 entries per problem)
    int ccam_off;       // into cc_start (nfc + 1 entries per problem): the per-camera lists of cam_part partial sums
    int be_nch;         // device-built block entries: 64-item chunks of the longest camera list
    int becnt_off;      // ... and this problem's [nfc][be_nch][nfc] counters
    double K[4];
    double bf;
};

struct Opt
{
    int max_pcg;
    int pcg_general;  // SNK_BA_PCG_GENERAL=1: the 256-thread PCG loop for every size (A/B against the replicated one)
    double pcg_tol, huber_mono, huber_stereo, lambda_init;
    double chi2_mono, chi2_stereo;  // point_pass<3> (the chi-square pass of SolveLocalScene): thresholds of the squared residual
};

struct State  // per problem, device resident
{
    double cost, cost_new, lambda, vfac, cost_initial;
    int accepted, iter, pcg_iters;
    int marked;  // observations the chi-square pass after this solve marked (point_pass<3>); begin_solve resets it
    double first_cost_initial, first_cost;  // the costs at the time of that pass (a conditional extra iteration overwrites the others)
};

struct RpcMeta
{
    int img1, img2;  // image index inside the problem
    int c1, c2;      // free-camera index or -1
    double rel[7];
    double w_rot, w_trans;
};
constexpr int RPC_STRIDE = 72;

// What cam_pass needs of an observation that never changes during a solve, stored in the order of the camera lists
// so that a camera's workgroup streams it: 40 bytes (round 5; 48 before: cam_pass and update_cost run at the speed their records
// stream at, so the index fields are packed -- the point index and "the point is an unknown" share a word, the image is the
// camera's and is looked up once per camera).
struct CamObs
{
    double u, v, depth, weight;
    int ptw;   // point index | "the point is an unknown" << 31
    int orig;  // caller-order index (global)
};

// One wavefront's share of the point-major Schur pass: <= SET_CHUNK points that are all observed by the same cameras
// in the same order (same "camera set"), so that lane q owns pair slot q = rows (ra, rb) of a point's run for all of
// them and the 6 x 6 sum of block (camera(ra), camera(rb)) stays in its registers.
struct SetItem
{
    int pts_off, n_pts;    // into set_pts; n_pts <= SET_CHUNK <= 64 (one list entry per lane)
    int pair_off, npairs;  // into set_pairs: ra | rb << 8, camera(ra) < camera(rb) or ra == rb
    int part_off;          // first of its npairs partial sums in s_part (36 doubles each)
    int run;               // observations per point of this set
    int nfree;             // free-camera observations per point (k)
    int aux_off;           // into set_pairs: k run positions ordered by camera index, then the k x k table "pair slot of (i, j)", i <= j
    int rec_off;           // into set_obs: n_pts x run static observation records in (point of the item, observation) order
    int cpart_off;         // first of its nfree per-camera partial sums in cam_part (schur_fused<3, true>; 33 doubles each)
};

// camera sums of schur_fused<3, true>: 33 terms per (work item, free camera), in passes of eight: 0..7, 8..15, 16..23,
// 24..26 (from J_c and r) and 27..32 (W V^-1 b_p)
constexpr int CS_TERMS = 33, CS_PASSES = 5;

// Static part of an observation in the order schur_fused walks it (item, point of the item, observation of the point): a lane's
// record is at rec_off + group * run + lane, so the first round of loads of a group is three coalesced 16-byte loads.
// In memory 40 bytes (round 5; 48 before): image, free-camera index and the "unknown" flag share a word.  SET_MAX_IMG bounds the images of a
// problem for which the packed form exists (snk_ba_set_problems refuses more).
constexpr int SET_MAX_IMG = 32767;
struct SetObs
{
    double u, v, depth, weight;
    int orig;  // caller-order index (global)
    int pk;    // image inside the problem (15 bits) | point is an unknown << 15 | (free-camera index + 1) << 16
};
__host__ __device__ inline int set_pack(int img, int cam, int ptfree) { return img | (ptfree ? 1 << 15 : 0) | ((cam + 1) << 16); }

struct Arrays
{
    const Prob* prob;
    State* state;
    double* pose;  // [img][7]
    double* pose_new;
    double* pt;  // [pt][3]
    double* pt_new;
    const unsigned char* pt_const;
    const int* cam_idx;  // [img] free-camera index or -1
    const int* pt_start;
    // observations sorted by point
    const int* o_img;
    const int* o_cam;               // free-camera index of the observation's image, or -1
    const unsigned char* o_ptfree;  // 1 when the observation's point is an unknown
    const double2* o_uv;
    const double* o_depth;
    const double* o_weight;
    const int* o_orig;             // caller-order index (global over problems)
    const int* o_pt;               // point index (inside the problem) of the observation
    const int* wv_pt;              // [n_wv + 1] per problem: first point of every point_wave work item
    // relative pose constraints
    const RpcMeta* rpc_meta;       // [rpc]
    double* rpc_out;               // [rpc][RPC_STRIDE]: cost, trial cost, g1[6], g2[6], H11 upper[21], H12[36]
    const int* cam_rpc_start;      // [nfc + 1] per problem
    const int* cam_rpc_items;      // rpc index (inside the problem) * 2 + side (0: the camera is img1, 1: img2)
    const int* blk_rpc;            // [nfc * nfc] per problem (at blkstart_off - problem index): 0 or 1 + (rpc * 2 + transposed)
    const int* rpc_next;           // [rpc] chain of further constraints on the same camera pair, same encoding
    const unsigned char* outlier;  // caller order
    double* o_r;   // [obs][4]  scaled residual, [3] = dim (0: inactive in this iteration)
    double* o_W;   // [obs][18]
    double* ptv;   // [pt][6]   point position of the linearisation | V^-1 b_p (cam_pass rebuilds J_c, r, Y b_p from them)
    const CamObs* cs_obs;  // static observation records in camera order (indexed like cam_items)
    double* Vinv;  // [pt][6]
    double* bp;    // [pt][3]
    double* cost_pt;
    double* cost_pt_new;
    double* U;  // [cam][36] damped
    const int* cam_start;
    const int* cam_items;
    const int* blk_start;
    const int4* blk_ent;  // (observation of c1, observation of c2, point, 0), observation indices relative to the problem
    const SetItem* set_items;
    const int2* set_pts;  // (point, first observation of the point) inside the problem
    const int* set_pairs;
    const SetObs* set_obs;
    const int* cblk_start;  // per problem, per block: its partial sums in cblk_items (fixed order)
    const int* cblk_items;  // index into s_part
    double* s_part;         // [partial][36]
    const int* cc_start;    // per problem, per free camera: its per-item partial sums in cc_items (fixed order)
    const int* cc_items;    // index into cam_part
    double* cam_part;       // [partial][33]: b_c (6) | U upper (21) | Y b_p (6) of one camera over one work item's points
    double* S;
    double* rhs;
    double* x;
    double* chi2;  // caller order
};

// ---- limits of the point-major Schur pass (schur_set / schur_mfma / schur_fused in ba.hip; the hand-over cuts the work items to them) ----
constexpr int SET_CHUNK   = 50;  // points per work item (a set's points are cut into equal items of at most this many)
// Big batches (>= 256 problems, every set with <= 8 free cameras, default kernels): items of up to 128 points.  Every item
// writes one 288-byte partial sum per camera pair whatever its size: with 100 points per camera set (the benchmark window) one
// item per set instead of two halves what schur_fused writes and schur_sum reads back (425 MB per LM iteration of 1024 windows).
// Only schur_fused / update_cost walk such items (two list registers); the alternative paths keep <= 64.
constexpr int SET_CHUNK_BIG = 104;
constexpr int SET_MAX_RUN = 14;  // observations of a point (rows staged per point)
constexpr int SET_MAX_K   = 10;  // free-camera observations of a point: 55 pairs <= 64 lanes

// Work arrays of the PCG forms for reduced systems that do not fit one workgroup's LDS (pcgl_*, imp_* in ba.hip), carved from
// d_pcgw by ba_plan_pcg.
struct PcgLarge
{
    double* r;     // [tot_vec]
    double* z;
    double* p;
    double* Ap;
    double* Minv;  // [tot_cam][36]
    double* ps;    // [parts][tot_vec]
    double* prr;   // [2][B][G] partial r.r   (double-buffered by iteration parity)
    double* prz;   // [2][B][G] partial r.z
    double* ppap;  // [B][G]    partial p.Ap
    double* scal;  // [B][4]    stop2, done, -, -
    int G, parts, tot_vec, B;
    // the one-launch form (pcgl_persist, one problem): p double-buffered, per-workgroup partial sums, the grid barrier's counter
    double* p2;       // [tot_vec]  the other direction buffer
    double* wrr;      // [2][PERSIST_WGS]  partial r.r  (by iteration parity)
    double* wrz;      // [2][PERSIST_WGS]  partial r.z
    double* wpap;     // [PERSIST_WGS]     partial p.Ap
    unsigned* bar;    // [BAR_WORDS] the grid barrier's phase flags: per workgroup, per group of eight, per group generation (zeroed by pcgl_init)
    int bar_flat;     // SNK_BA_FLAT_BARRIER=1: every workgroup polls every flag (the round-5 barrier)
    int persist_one;  // pcgl_persist1 (one grid barrier per PCG iteration; r, z, p private in LDS) instead of pcgl_persist
    int persist_wgs;  // workgroups of the launch (all resident: cooperative launch)
    int persist_rows;  // pcgl_persist_reg: rows of S per workgroup (8 or 16)
    int timing;       // SNK_BA_PCG_TIMING=1 (diagnostic): workgroup 0 of pcgl_persist_reg adds its cycles per phase to ps[0..5]
    double* y;        // implicit Schur form: [tot_pt][3] V^-1 W^T p of the point phase (ps[c] then holds p_c . (S p)_c)
    int zero_rows;    // implicit Schur form: point_wave linearised (inactive observations have zero W rows, o_r is not written)
};

// The lists a scene hand-over builds on the host live in PINNED vectors that belong to the handle and keep their capacity from call to
// call: hipMemcpyAsync from pageable memory stages and synchronises (33 uploads cost 0.23 ms per local-BA scene), from pinned memory
// it is an enqueue; and a new scene per keyframe no longer allocates and first-touches a megabyte of host memory.
template <typename T>
struct PinnedAlloc
{
    using value_type = T;
    PinnedAlloc() = default;
    template <typename U>
    PinnedAlloc(const PinnedAlloc<U>&) {}
    T* allocate(size_t n)
    {
        void* p = nullptr;
        if (hipHostMalloc(&p, n * sizeof(T), hipHostMallocDefault) != hipSuccess) throw std::bad_alloc();
        return static_cast<T*>(p);
    }
    void deallocate(T* p, size_t) { (void)hipHostFree(p); }
    // resize() default-initialises (no zero fill): every list is written in full right after it is sized, and zeroing hundreds of
    // megabytes of pinned memory first was host time of a batch hand-over; resize(n, value) still fills
    template <typename U>
    void construct(U* p) noexcept
    {
        ::new (static_cast<void*>(p)) U;
    }
    template <typename U, typename... Args>
    void construct(U* p, Args&&... args)
    {
        ::new (static_cast<void*>(p)) U(std::forward<Args>(args)...);
    }
    template <typename U>
    bool operator==(const PinnedAlloc<U>&) const { return true; }
    template <typename U>
    bool operator!=(const PinnedAlloc<U>&) const { return false; }
};
template <typename T>
using pvec = std::vector<T, PinnedAlloc<T>>;

struct BaLists
{
    pvec<Prob> probs;
    pvec<double> pose, pt, ouv2, odepth, oweight;
    pvec<unsigned char> ptc, optfree;
    pvec<SetItem> setitems;
    pvec<int2> setpts;
    pvec<int> setpairs, cblkstart, cblkitems, ccstart, ccitems;
    pvec<int> camidx, ptstart, oimg, ocam, oorig, camstart, camitems, blkstart, optidx, wvpt, rpcnext, camrpcstart, camrpcitems, blkrpc;
    pvec<RpcMeta> rpcmeta;
    pvec<int4> blkent;
    pvec<State> states;
    // snk_ba_set_problems_dev: the per-problem records to and from ho_count_kernel / ho_fill_kernel, the constant-image flags and the
    // constraint rows read back for the host stages (sized and written by the call itself: clear() leaves them alone)
    pvec<HoPlace> hoplace;
    pvec<HoOut> hoout;
    pvec<unsigned char> imgc;
    pvec<snk_ba_rpc> rpcrows;
    void clear()
    {
        probs.clear(), pose.clear(), pt.clear(), ouv2.clear(), odepth.clear(), oweight.clear(), ptc.clear(), optfree.clear();
        setitems.clear(), setpts.clear(), setpairs.clear(), cblkstart.clear(), cblkitems.clear();
        camidx.clear(), ptstart.clear(), oimg.clear(), ocam.clear(), oorig.clear(), camstart.clear(), camitems.clear();
        blkstart.clear(), optidx.clear(), wvpt.clear(), rpcnext.clear(), camrpcstart.clear(), camrpcitems.clear(), blkrpc.clear();
        rpcmeta.clear(), blkent.clear(), ccstart.clear(), ccitems.clear();
    }
};

// The host threads of a batch hand-over, kept by the handle (round 6, late).  snk_ba_set_problems runs seven threaded passes over the
// problems of a batch; with std::thread created and joined per pass that was 7 x 31 creations (~20 us each, issued one after the
// other) inside a 22 ms hand-over.  Workers park on a condition variable between passes and end with the handle.
constexpr int BA_FILL_CHUNKS = 4;   // chunks of problems the fill pass of a batch hand-over runs (and uploads) in
struct HostPool
{
    std::vector<std::thread> th;
    std::mutex m;
    std::condition_variable cv, cv_done;
    const std::function<void()>* job = nullptr;
    unsigned gen = 0;
    int n_run = 0, n_left = 0;
    bool stop = false;
    void worker(int idx)
    {
        unsigned seen = 0;
        for (;;)
        {
            const std::function<void()>* j = nullptr;
            {
                std::unique_lock<std::mutex> lk(m);
                cv.wait(lk, [&] { return stop || gen != seen; });
                if (stop) return;
                seen = gen;
                if (idx < n_run) j = job;
            }
            if (j)
            {
                (*j)();  // the passes catch their own exceptions
                std::lock_guard<std::mutex> lk(m);
                if (--n_left == 0) cv_done.notify_one();
            }
        }
    }
    // runs `work` on up to `helpers` pool threads and on the caller; returns when all of them are done
    void run(int helpers, const std::function<void()>& work)
    {
        try
        {
            while ((int)th.size() < helpers) th.emplace_back(&HostPool::worker, this, (int)th.size());
        }
        catch (...)
        {
        }  // thread creation failed: the threads that exist (and the caller) do the work
        const int n = std::min(helpers, (int)th.size());
        if (n > 0)
        {
            std::lock_guard<std::mutex> lk(m);
            job    = &work;
            n_run  = n;
            n_left = n;
            ++gen;
        }
        if (n > 0) cv.notify_all();
        work();
        if (n > 0)
        {
            std::unique_lock<std::mutex> lk(m);
            cv_done.wait(lk, [&] { return n_left == 0; });
            job = nullptr;
        }
    }
    ~HostPool()
    {
        {
            std::lock_guard<std::mutex> lk(m);
            stop = true;
        }
        cv.notify_all();
        for (auto& t : th) t.join();
    }
};

struct Handle : HandleBase
{
    BaLists lists;
    HostPool pool;    // host threads of the batch hand-over
    HostBuf h_stage;  // pinned staging of the small per-call transfers (outlier masks)
    DevBuf d_becnt;   // per (camera, 64-item chunk, camera) counters of the device-built block entries
    DevBuf d_probcond;  // the problem table of a conditional extra iteration (select_marked)
    DevBuf d_hoplace, d_hoout;  // HoPlace / HoOut per problem (snk_ba_set_problems_dev)
    DevBuf d_campart, d_ccstart, d_ccitems;  // per (work item, free camera) sums of schur_fused<3, true> and the per-camera lists of them
    bool state_fresh = false;                // the device state is the uploaded initial one (no solve since the hand-over)
    bool blk_built = true;                   // the camera-pair block entries of the current problem set exist on the device (see ba_sets_will_run)
    bool cam_sums_ok = false;                // every observation of a free camera belongs to a work item with pairs (no constant point seen by a free camera)
    snk_ba_options opt{};
    int count = 0;
    std::vector<Prob> probs;
    int tot_img = 0, tot_pt = 0, tot_obs = 0, tot_cam = 0, tot_orig = 0, tot_vec = 0;
    long long tot_s = 0;
    int max_np = 0, max_nfc = 0, max_n6 = 0, max_ni = 0, max_set_items = 0;
    bool set_ok = false, set_small = false;
    int set_k_max = 0, set_run_max = 0;
    DevBuf d_setitems, d_setpts, d_setpairs, d_setobs, d_cblkstart, d_cblkitems, d_spart;
    DevBuf d_prob, d_state, d_pose, d_pose_new, d_pose0, d_pt, d_pt_new, d_pt0, d_ptc, d_camidx, d_ptstart, d_oimg, d_ocam,
        d_optfree, d_ouv, d_odepth, d_oweight, d_oorig, d_outlier, d_csobs, d_r, d_W, d_ptv, d_Vinv, d_bp, d_cost,
        d_cost_new, d_U, d_camstart, d_camitems, d_blkstart, d_blkent, d_S, d_rhs, d_x, d_chi2, d_pcgw, d_optidx, d_wvpt, d_rpcmeta, d_rpcnext, d_camrpcstart, d_camrpcitems, d_blkrpc, d_rpcout;
    int max_rpc = 0;
    int max_wv = 0;
    bool point_wave_ok = false;  // every problem has a point_wave work list (no point with > 64 observations)
    PcgLarge pcgw{};     // work arrays of the multi-workgroup PCG (only when the reduced system exceeds the LDS)
    bool pcg_large = false;
    int explicit_schur = 1;  // snk_ba_set_explicit_schur: the form the next hand-over builds
    bool implicit = false;   // the current problem set runs the implicit Schur form (imp_*): no S, no camera-pair lists
    Arrays arr{};
    std::vector<int> orig_off, orig_n;
    std::map<int, hipGraphExec_t> graphs;  // LM launch sequence captured per iteration count
    std::map<int, int> plain_runs;         // solves issued with plain launches since set_problems, per iteration count
    void drop_graphs()
    {
        for (auto& g : graphs) (void)hipGraphExecDestroy(g.second);
        graphs.clear();
        plain_runs.clear();
    }
};

// The hand-over's lists reach the device with ONE kernel that reads the pinned host vectors over the bus (hipHostMalloc memory is
// device-visible) and writes the device arrays: 33 separate copies cost ~6 us each on the copy engine whatever their size.
constexpr int COPY_TAB_MAX = 48;
struct CopyTab
{
    const void* src[COPY_TAB_MAX];
    void* dst[COPY_TAB_MAX];
    unsigned bytes[COPY_TAB_MAX];
    int n;
};
}  // namespace ba
}  // namespace snk

struct snk_ba : snk::ba::Handle  // the C ABI's opaque handle (snake_hip.h)
{
};

namespace snk
{
namespace ba
{
// ---- ba.hip, called by the hand-over ----
Opt make_opt(const snk_ba_options& o);
// The ONE reader of the solver's switches (BaSwitches in dispatch.hpp names each), filled at the first use in a process.
inline const BaSwitches& ba_switches()
{
    static const BaSwitches once = []
    {
        const auto on  = [](const char* name) { return getenv(name) != nullptr; };
        const auto num = [](const char* name) { const char* e = getenv(name); return e && atoi(e) > 0 ? atoi(e) : 0; };
        BaSwitches s;
        s.pcg_general          = on("SNK_BA_PCG_GENERAL");
        s.no_point_wave        = on("SNK_BA_NO_POINT_WAVE");
        s.no_schur_set         = on("SNK_BA_NO_SCHUR_SET");
        if (const char* e = getenv("SNK_BA_SCHUR_SET_MIN_ITEMS")) s.set_min_items = atoll(e);
        s.no_schur_mfma        = on("SNK_BA_NO_SCHUR_MFMA");
        s.no_schur_fused       = on("SNK_BA_NO_SCHUR_FUSED");
        s.fused_k10            = on("SNK_BA_FUSED_K10");
        s.cam_sums             = on("SNK_BA_CAM_SUMS");
        s.cam_grid_2d          = on("SNK_BA_CAM_GRID_2D");
        s.no_schur_wide        = on("SNK_BA_NO_SCHUR_WIDE");
        s.pcg_lds              = on("SNK_BA_PCG_LDS");
        s.no_update_cost       = on("SNK_BA_NO_UPDATE_COST");
        s.flat_barrier         = on("SNK_BA_FLAT_BARRIER");
        s.pcg_timing           = on("SNK_BA_PCG_TIMING");
        s.pcgl_launches        = on("SNK_BA_PCGL_LAUNCHES");
        s.persist_two_barriers = on("SNK_BA_PERSIST_TWO_BARRIERS");
        s.persist_stream       = on("SNK_BA_PERSIST_STREAM");
        s.persist_wgs          = on("SNK_BA_PERSIST_WGS") ? num("SNK_BA_PERSIST_WGS") : -1;
        s.persist_reg_rows     = num("SNK_BA_PERSIST_REG_ROWS");
        s.persist_fail         = on("SNK_BA_PERSIST_FAIL");
        s.graph_chains         = num("SNK_BA_GRAPH_CHAINS");
        s.no_graph             = on("SNK_BA_NO_GRAPH");
        s.graph_first          = on("SNK_BA_GRAPH_FIRST");
        s.local_sync           = on("SNK_BA_LOCAL_SYNC");
        s.debug                = on("SNK_DEBUG");
        return s;
    }();
    return once;
}
// The totals of the handle's problem set that dispatch.hpp's rules decide on
inline BaShape ba_shape(const snk_ba* h)
{
    BaShape s;
    s.count = h->count, s.implicit = h->implicit;
    s.max_n6 = h->max_n6, s.max_nfc = h->max_nfc, s.max_np = h->max_np, s.max_ni = h->max_ni, s.max_wv = h->max_wv, s.max_rpc = h->max_rpc;
    s.max_set_items = h->max_set_items;
    s.set_ok = h->set_ok, s.set_small = h->set_small, s.set_k_max = h->set_k_max, s.set_run_max = h->set_run_max;
    s.point_wave_ok = h->point_wave_ok, s.cam_sums_ok = h->cam_sums_ok, s.blk_built = h->blk_built;
    s.persist_wgs = h->pcgw.persist_wgs, s.persist_one = h->pcgw.persist_one, s.persist_rows = h->pcgw.persist_rows;
    return s;
}
// Will the LM sequence of this problem set run the point-major kernels?  dispatch.hpp's ba_sets_will_run on the handle's shape and
// the process's switches: the hand-over leaves out the block entries on the answer the solver will plan by
bool ba_sets_will_run(const snk_ba* h);
// The PCG form of the problem set and its work arrays.  Called by the hand-over once the totals of the set are in the handle
// (count, implicit, max_n6, max_nfc, max_np, tot_vec, tot_cam, tot_pt): sets pcg_large and pcgw, reserves d_pcgw.
int ba_plan_pcg(snk_ba* h);
// ---- ba_handover.hip, called by the solver ----
// copy_table_kernel over the entries of `tab` (gx workgroups per entry) on `stream`: snk_ba_solve_local_scene returns its results with it
int ba_copy_table(const CopyTab& tab, int gx, hipStream_t stream);
}  // namespace ba
}  // namespace snk
