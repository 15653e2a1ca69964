// Driver of snake_hip::PoseGraph / PGORec / PGOSim3Rec / TransformMapPoints: reads a graph from a directory (poses.bin [n, 8], constant.bin
// [n] as doubles, edges.bin [E, 3] doubles (i, j, weight) in the order they are added, set_pose.bin [9] = vertex + Sim3, params.bin =
// {fix_scale}, points.bin [m, 4] = reference vertex + position), runs it as OptimizeEssentialGraph does and writes the result.
#include <cstdio>
#include <string>
#include <vector>

#include "snake_hip.hpp"

static std::vector<double> load(const std::string& path)
{
    std::vector<double> v;
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) throw std::runtime_error("pgo_driver: missing input " + path);
    double x;
    while (fread(&x, 8, 1, f) == 1) v.push_back(x);
    fclose(f);
    return v;
}
static void store(const std::string& path, const std::vector<double>& v)
{
    FILE* f = fopen(path.c_str(), "wb");
    if (!f || fwrite(v.data(), 8, v.size(), f) != v.size()) throw std::runtime_error("pgo_driver: cannot write " + path);
    fclose(f);
}

template <class Rec>
static void run(const std::string& dir, snake_hip::PoseGraph& pg, const std::vector<double>& pts)
{
    Rec rec;
    rec.optimizationOptions.max_iterations = 50;
    rec.optimizationOptions.min_chi2_delta = 1e-10;
    rec.create(pg);
    const snk_pgo_result r = rec.initAndSolve();
    std::vector<double> out;
    for (const auto& T : rec.poses()) out.insert(out.end(), T.begin(), T.end());
    store(dir + "/out_poses.bin", out);
    store(dir + "/out_result.bin", {r.cost_initial, r.cost_final, (double)r.lm_iterations, (double)r.pcg_iterations_total, (double)r.accepted_steps});
    const size_t m = pts.size() / 4;
    std::vector<int32_t> ref(m);
    std::vector<std::array<double, 3>> pos(m), nrm;
    std::vector<double> depth(m, 2.0);
    for (size_t k = 0; k < m; ++k) ref[k] = (int32_t)pts[4 * k], pos[k] = {pts[4 * k + 1], pts[4 * k + 2], pts[4 * k + 3]};
    snake_hip::TransformMapPoints(rec, ref, pos, nrm, depth);
    out.clear();
    for (size_t k = 0; k < m; ++k) out.insert(out.end(), {pos[k][0], pos[k][1], pos[k][2], depth[k]});
    store(dir + "/out_points.bin", out);
}

int main(int argc, char** argv)
{
    try
    {
        const std::string dir = argc > 1 ? argv[1] : ".";
        const auto poses = load(dir + "/poses.bin"), cst = load(dir + "/constant.bin"), ed = load(dir + "/edges.bin"), sp = load(dir + "/set_pose.bin"),
                   par = load(dir + "/params.bin"), pts = load(dir + "/points.bin");
        const size_t n = cst.size();
        if (poses.size() != n * 8 || sp.size() != 9 || par.size() != 1 || ed.size() % 3 || pts.size() % 4) throw std::runtime_error("pgo_driver: bad input sizes");
        std::vector<snake_hip::PoseGraph::Sim3> P(n);
        std::vector<uint8_t> C(n);
        for (size_t v = 0; v < n; ++v)
        {
            for (int k = 0; k < 8; ++k) P[v][(size_t)k] = poses[v * 8 + (size_t)k];
            C[v] = cst[v] != 0.0;
        }
        snake_hip::PoseGraph pg(P, C, par[0] != 0.0);
        for (size_t e = 0; e < ed.size() / 3; ++e) pg.AddVertexEdge((int)ed[3 * e], (int)ed[3 * e + 1], ed[3 * e + 2]);
        pg.sortEdges();
        snake_hip::PoseGraph::Sim3 T;
        for (int k = 0; k < 8; ++k) T[(size_t)k] = sp[1 + (size_t)k];
        pg.SetPose((int)sp[0], T);
        if (pg.fixScale)
            run<snake_hip::PGORec>(dir, pg, pts);
        else
            run<snake_hip::PGOSim3Rec>(dir, pg, pts);
        return 0;
    }
    catch (const std::exception& e)
    {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
}
