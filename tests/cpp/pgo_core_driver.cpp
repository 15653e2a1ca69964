// g++-only driver of pgo_core.hpp: reads a directory of edges (Ti, Tj, M [E, 8] doubles, weights [E], params.bin = {E, D}), writes the
// residual, the two Jacobians and the block products of every edge.  tests/test_pgo_core_cpu.py compares them with the numpy restatement.
#include <cstdio>
#include <string>
#include <vector>

#include "pgo_core.hpp"

static std::vector<double> load(const std::string& path)
{
    std::vector<double> v;
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) return v;
    double x;
    while (fread(&x, 8, 1, f) == 1) v.push_back(x);
    fclose(f);
    return v;
}
static bool store(const std::string& path, const std::vector<double>& v)
{
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) return false;
    const bool ok = fwrite(v.data(), 8, v.size(), f) == v.size();
    fclose(f);
    return ok;
}

int main(int argc, char** argv)
{
    if (argc < 2) return 2;
    const std::string dir = argv[1];
    const auto par = load(dir + "/params.bin");
    const auto Ti = load(dir + "/Ti.bin"), Tj = load(dir + "/Tj.bin"), M = load(dir + "/M.bin"), w = load(dir + "/w.bin");
    if (par.size() != 2) return 3;
    const int E = (int)par[0], D = (int)par[1];
    if ((int)w.size() != E || (int)Ti.size() != E * 8 || (int)Tj.size() != E * 8 || (int)M.size() != E * 8) return 4;
    std::vector<double> r(E * 7), Ji(E * 49), Jj(E * 49), Hii(E * 49), Hij(E * 49), Hjj(E * 49), gi(E * 7), gj(E * 7), rt(E * 8);
    for (int e = 0; e < E; ++e)
    {
        double ws[3 * 49];
        pgo::Mat<1> N{ws}, P{ws + 49}, S{ws + 98};
        pgo::edge_jacobians(&Ti[e * 8], &Tj[e * 8], &M[e * 8], w[e], D, &r[e * 7], N, P, S);
        for (int k = 0; k < 49; ++k) Ji[e * 49 + k] = P.p[k], Jj[e * 49 + k] = S.p[k];
        pgo::at_b(P, P, &Hii[e * 49]);
        pgo::at_b(P, S, &Hij[e * 49]);
        pgo::at_b(S, S, &Hjj[e * 49]);
        pgo::at_r(P, &r[e * 7], &gi[e * 7]);
        pgo::at_r(S, &r[e * 7], &gj[e * 7]);
        pgo::retract(&Ti[e * 8], &r[e * 7], D, &rt[e * 8]);  // T_i . exp(r): the update's statement on the same inputs
    }
    const bool ok = store(dir + "/out_r.bin", r) && store(dir + "/out_Ji.bin", Ji) && store(dir + "/out_Jj.bin", Jj) && store(dir + "/out_Hii.bin", Hii) &&
                    store(dir + "/out_Hij.bin", Hij) && store(dir + "/out_Hjj.bin", Hjj) && store(dir + "/out_gi.bin", gi) && store(dir + "/out_gj.bin", gj) &&
                    store(dir + "/out_retract.bin", rt);
    return ok ? 0 : 5;
}
