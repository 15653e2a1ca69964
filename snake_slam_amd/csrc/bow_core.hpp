// "snk-bow v1" (DESIGN.md section 3g): the statements of the bag-of-words place recognition that decide a result -- the descent step
// of the vocabulary transform (Snake/Map/Frame.cpp:38-40; Saiga::MiniBow2 is absent, the rule is DBoW2's published one and [DEFINED]),
// the per-word term of the L1 score (LoopDetector.cpp:73), the filters of KeyframeDatabase::RemoveWeakMatches
// (Snake/LoopClosing/KeyframeDatabase.cpp:123-168) and the candidate update and accept rule of LoopORBmatcher::MatchBoW
// (Snake/LoopClosing/LoopORBMatcher.cpp:156-196) -- as functions of plain values, so that the kernels (bow.hip) and a plain g++ build
// (tests/cpp/bow_core_driver.cpp) run the same text.  Integers and comparisons only, apart from the score term (one subtraction, one
// fabs, two subtractions in double) and the two float products of the filters.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define SNK_BOW_HD __host__ __device__ __forceinline__
#else
#define SNK_BOW_HD inline
#endif

namespace snk
{
constexpr int BOW_MAX_DEPTH    = 16;    // of a vocabulary tree (root = depth 0)
constexpr int BOW_MAX_FEATURES = 2048;  // per frame; also the most words of a query or a database row
constexpr int BOW_MAX_CANDIDATES = 64;  // a query returns at most this many keyframes

// The vocabulary as the kernels walk it: the children of a node are contiguous ("slots" first .. first + count), each slot holds the
// child's node id and its descriptor.
struct BowTree
{
    const int32_t* first;      // [n_nodes] first child slot
    const int32_t* count;      // [n_nodes] children; 0 = leaf
    const int32_t* slot_node;  // [n_slots] node id of the child in this slot
    const uint64_t* slot_desc; // [n_slots][4]
    const int32_t* word;       // [n_nodes] dense word id of a leaf, -1 inside
    const double* weight;      // [n_nodes] leaves only
    int32_t depth;             // L: depth of the deepest leaf (validated, <= BOW_MAX_DEPTH)
};

SNK_BOW_HD int bow_popcount64(uint64_t x)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __popcll(x);
#else
    return __builtin_popcountll(x);
#endif
}

SNK_BOW_HD int bow_distance(const uint64_t* a, const uint64_t* b)
{
    return bow_popcount64(a[0] ^ b[0]) + bow_popcount64(a[1] ^ b[1]) + bow_popcount64(a[2] ^ b[2]) + bow_popcount64(a[3] ^ b[3]);
}

// The key of child number `c` (position in the node's child list) at Hamming distance `dist`: the smallest key is the child the
// descent takes -- the smallest distance, and of equal distances the first child (strict < in list order).  dist <= 256, c < 2^20.
SNK_BOW_HD uint32_t bow_child_key(int dist, int c)
{
    return ((uint32_t)dist << 20) | (uint32_t)c;
}
constexpr uint32_t BOW_NO_CHILD = 0xffffffffu;

// One descent step as a serial statement: the slot of the child of `node` nearest to d.  node must not be a leaf.
SNK_BOW_HD int bow_descend_step(const BowTree& T, int node, const uint64_t* d)
{
    const int first = T.first[node], count = T.count[node];
    uint32_t best = BOW_NO_CHILD;
    for (int c = 0; c < count; ++c)
    {
        const uint32_t k = bow_child_key(bow_distance(d, T.slot_desc + (size_t)(first + c) * 4), c);
        best             = k < best ? k : best;
    }
    return first + (int)(best & 0xfffffu);
}

// The depth at which the feature vector's node is taken; <= 0: no feature vector (every feature records node 0)
SNK_BOW_HD int bow_node_depth(int L, int levelsup)
{
    return L - levelsup;
}

// Transform of one descriptor: word = the leaf's dense id, node = the node of the path at depth L - levelsup, 0 when that depth is
// <= 0 or the path ends above it.  The loop is bounded by the validated depth.
SNK_BOW_HD void bow_transform_one(const BowTree& T, const uint64_t* d, int levelsup, int& leaf, int& node_up)
{
    const int target = bow_node_depth(T.depth, levelsup);
    int node = 0;
    node_up  = 0;
    for (int depth = 1; depth <= T.depth; ++depth)
    {
        if (T.count[node] == 0) break;
        node = T.slot_node[bow_descend_step(T, node, d)];
        if (depth == target) node_up = node;
    }
    leaf = node;
}

// -1/2 of this, summed over the common words, is the L1 score of two normalised vectors (in [0, 1])
SNK_BOW_HD double bow_score_term(double a, double b)
{
    return fabs(a - b) - a - b;
}

// RemoveWeakMatches, KeyframeDatabase.cpp:137: `mnLoopWords < sharing_word_ratio * maxCommonWords` (int * float -> float)
SNK_BOW_HD bool bow_too_few_common(int common, float sharing_word_ratio, int max_common)
{
    return (float)common < sharing_word_ratio * (float)max_common;
}

// KeyframeDatabase.cpp:158-159 with the scores kept in double [DEFINED]
SNK_BOW_HD bool bow_score_too_low(double score, float score_ratio, double best, float min_score)
{
    return score < (double)score_ratio * best || score < (double)min_score;
}

// order of the candidates: score descending, ties to the lower keyframe id [DEFINED]
SNK_BOW_HD bool bow_candidate_before(double sa, int ida, double sb, int idb)
{
    return sa > sb || (sa == sb && ida < idb);
}

// MatchBoW keeps the two smallest distances of a feature's candidates (LoopORBMatcher.cpp:174-183).  As a key (dist << 16 | position
// in the node's keyframe-2 list) the best candidate is the smallest key -- strict <: the first of minimal distance -- and the second
// distance is the distance of the second smallest key.  Both start at 256 (:156-158).
constexpr uint32_t BOW_MATCH_NONE = (256u << 16) | 0xffffu;
SNK_BOW_HD uint32_t bow_match_key(int dist, int pos)
{
    return ((uint32_t)dist << 16) | (uint32_t)pos;
}
SNK_BOW_HD void bow_match_update(uint32_t key, uint32_t& k1, uint32_t& k2)
{
    // `if (key < k1) { k2 = k1; k1 = key; } else if (key < k2) k2 = key;` without branches (the compiler kept k1 / k2 in memory otherwise)
    const uint32_t lo = key < k1 ? key : k1, hi = key < k1 ? k1 : key;
    k1 = lo;
    k2 = hi < k2 ? hi : k2;
}
// LoopORBMatcher.cpp:186-188
SNK_BOW_HD bool bow_match_accept(uint32_t k1, uint32_t k2, int threshold, float ratio)
{
    const int d1 = (int)(k1 >> 16), d2 = (int)(k2 >> 16);
    return d1 < threshold && (float)d1 < ratio * (float)d2;
}

// Validation of a vocabulary given as flat arrays (node 0 = root).  Returns NULL when the tree is sound, otherwise what is wrong.  On
// success *depth_out = L and *n_words_out = the number of leaves.  depth_of (n_nodes ints) is scratch the caller provides.
inline const char* bow_validate(int n_nodes, const int32_t* child_start, const int32_t* child_count, const int32_t* children, int n_children,
                                const int32_t* word_id, const double* weight, int32_t* depth_of, int* depth_out, int* n_words_out)
{
    if (n_nodes < 1 || n_children < 0) return "a vocabulary needs at least the root";
    if (n_children != n_nodes - 1) return "every non-root node must be the child of exactly one node (children != nodes - 1)";
    for (int i = 0; i < n_nodes; ++i)
    {
        depth_of[i] = -1;
        if (child_count[i] < 0 || child_count[i] >= (1 << 20)) return "child_count outside [0, 2^20)";
        if (child_count[i] > 0 && (child_start[i] < 0 || (int64_t)child_start[i] + child_count[i] > n_children)) return "child list outside children[]";
    }
    // parents: each non-root node listed exactly once, the root never
    for (int i = 0; i < n_nodes; ++i)
        for (int c = 0; c < child_count[i]; ++c)
        {
            const int ch = children[child_start[i] + c];
            if (ch <= 0 || ch >= n_nodes) return "child id outside (0, n_nodes)";
            if (depth_of[ch] != -1) return "a node is the child of two nodes";
            depth_of[ch] = -2;  // has a parent
        }
    for (int i = 1; i < n_nodes; ++i)
        if (depth_of[i] != -2) return "orphan node: not a child of any node";
    // depths from the root, breadth first over the children lists; a node in a cycle is never reached
    depth_of[0] = 0;
    int reached = 1, L = 0;
    for (int d = 0; d <= BOW_MAX_DEPTH; ++d)
    {
        int found = 0;
        for (int i = 0; i < n_nodes; ++i)
        {
            if (depth_of[i] != d) continue;
            for (int c = 0; c < child_count[i]; ++c)
            {
                if (d == BOW_MAX_DEPTH) return "depth above 16";
                depth_of[children[child_start[i] + c]] = d + 1;
                ++found;
            }
            if (child_count[i] == 0 && d > L) L = d;
        }
        reached += found;
        if (found == 0) break;
    }
    if (reached != n_nodes) return "cycle: a node cannot be reached from the root";
    int n_words = 0;
    for (int i = 0; i < n_nodes; ++i) n_words += child_count[i] == 0 ? 1 : 0;
    for (int i = 0; i < n_nodes; ++i) depth_of[i] = 0;  // reused: how often word id i is taken (n_words <= n_nodes)
    for (int i = 0; i < n_nodes; ++i)
    {
        if (child_count[i] > 0)
        {
            if (word_id[i] != -1) return "an inner node carries a word id";
            continue;
        }
        if (word_id[i] < 0 || word_id[i] >= n_words) return "a leaf without a word id in [0, n_words)";
        if (depth_of[word_id[i]]++ != 0) return "a word id is used twice";
        if (!(weight[i] >= 0.0) || !std::isfinite(weight[i])) return "a weight that is negative or not finite";
    }
    *depth_out   = L;
    *n_words_out = n_words;
    return nullptr;
}
}  // namespace snk
