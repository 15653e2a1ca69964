// Runs snake_hip::LocalMapBuilder (snake_slam_amd/cpp/snake_hip.hpp) the way Snake's tracking loop would after the vote: the vote's
// lists as CovisibilityGraph::List, every keyframe's connections added keyframe by keyframe, the map side and the point table filled
// into LocalMapBuilder::Points, one Select and one Gather call.  Inputs and outputs are raw little-endian arrays in the directory
// argv[1] (written / read by tests/test_cpp_localmap_gpu.py, which compares the outputs with the restatement).
//   meta.bin (int32): n_sets, vote_cap, n_kf, n_direct, n_direct_prob, n_indirect_prob, n_neighbours, kf_cap, pts_cap, n_gather_sets
//   seed.bin (uint64); select: conn, vote, kf_bad, conn_start, conn_list, frame_id; gather: feat_start, feat_point, pt_flags,
//   pt_last_seen, pos, normal, desc, ref_depth, ref_level, g_frame_id, g_local_kf, g_sel, set_start, set_point
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "snake_hip.hpp"

static std::string g_dir;

template <typename T>
static std::vector<T> rd(const std::string& name)
{
    std::ifstream f(g_dir + "/" + name + ".bin", std::ios::binary | std::ios::ate);
    if (!f) throw std::runtime_error("missing input " + name);
    const size_t bytes = (size_t)f.tellg();
    if (bytes % sizeof(T)) throw std::runtime_error("size of " + name + " is not a multiple of its element size");
    std::vector<T> v(bytes / sizeof(T));
    f.seekg(0);
    f.read(reinterpret_cast<char*>(v.data()), (std::streamsize)bytes);
    return v;
}

template <typename T>
static void wr(const std::string& name, const std::vector<T>& v)
{
    std::ofstream f(g_dir + "/" + name + ".bin", std::ios::binary);
    f.write(reinterpret_cast<const char*>(v.data()), (std::streamsize)(v.size() * sizeof(T)));
}

using snake_hip::CovisibilityGraph;
using snake_hip::LocalMapBuilder;

int main(int argc, char** argv)
{
    if (argc != 2)
    {
        std::cerr << "usage: localmap_driver DIR\n";
        return 2;
    }
    g_dir = argv[1];
    try
    {
        const auto meta = rd<int32_t>("meta");
        const int n_sets = meta[0], vote_cap = meta[1], n_kf = meta[2], kf_cap = meta[7], pts_cap = meta[8], n_gsets = meta[9];
        const snk_lmap_params par{meta[3], meta[4], meta[5], meta[6], kf_cap, rd<uint64_t>("seed")[0]};
        LocalMapBuilder builder(par);

        // ---- stage 1: the lists as the vote returned them, the graph keyframe by keyframe ----
        const auto conn = rd<snk_covis_conn>("conn");
        const auto vote = rd<snk_covis_result>("vote");
        std::vector<CovisibilityGraph::List> votes((size_t)n_sets);
        for (int s = 0; s < n_sets; ++s)
        {
            const snk_covis_conn* row = conn.data() + (size_t)s * (size_t)vote_cap;
            votes[(size_t)s].connections.assign(row, row + vote[(size_t)s].n_conn);
            votes[(size_t)s].n_found = vote[(size_t)s].n_found;
            votes[(size_t)s].status  = vote[(size_t)s].status;
        }
        const auto kf_bad = rd<uint8_t>("kf_bad");
        const auto cs     = rd<int32_t>("conn_start");
        const auto cl     = rd<snk_covis_conn>("conn_list");
        LocalMapBuilder::Graph graph;
        for (int k = 0; k < n_kf; ++k) graph.AddKeyframe(kf_bad[(size_t)k] != 0, std::vector<snk_covis_conn>(cl.begin() + cs[(size_t)k], cl.begin() + cs[(size_t)k + 1]));
        const LocalMapBuilder::Selection sel = builder.Select(votes, graph, rd<int32_t>("frame_id"));
        wr("out_local_kf", sel.local_kf);
        wr("out_sel", sel.result);

        // ---- stage 2 on the gather case: its own local keyframes and records ----
        LocalMapBuilder::Points pts;
        pts.feat_start = rd<int32_t>("feat_start"), pts.feat_point = rd<int32_t>("feat_point"), pts.pt_flags = rd<uint8_t>("pt_flags");
        pts.pt_last_seen = rd<int32_t>("pt_last_seen"), pts.pos = rd<double>("pos"), pts.normal = rd<double>("normal"), pts.desc = rd<uint64_t>("desc");
        pts.ref_depth = rd<float>("ref_depth"), pts.ref_level = rd<int32_t>("ref_level");
        LocalMapBuilder::Selection gsel;
        gsel.local_kf = rd<int32_t>("g_local_kf");
        gsel.result   = rd<snk_lmap_select_result>("g_sel");
        const auto ss = rd<int32_t>("set_start");
        const auto sp = rd<int32_t>("set_point");
        std::vector<std::vector<int32_t>> own((size_t)n_gsets);
        for (int s = 0; s < n_gsets; ++s) own[(size_t)s].assign(sp.begin() + ss[(size_t)s], sp.begin() + ss[(size_t)s + 1]);
        const auto frames = builder.Gather(pts, gsel, rd<int32_t>("g_frame_id"), own, pts_cap);
        std::vector<snk_lm_fine> lm;
        std::vector<int32_t> ids, counts;
        std::vector<snk_lmap_gather_result> res;
        for (const auto& f : frames)
        {
            lm.insert(lm.end(), f.points.begin(), f.points.end());
            ids.insert(ids.end(), f.ids.begin(), f.ids.end());
            counts.push_back((int32_t)f.points.size());
            res.push_back(f.result);
        }
        wr("out_lm", lm);
        wr("out_ids", ids);
        wr("out_counts", counts);
        wr("out_res", res);
        return 0;
    }
    catch (const std::exception& e)
    {
        std::cerr << e.what() << "\n";
        return 1;
    }
}
