// CPU build of dispatch.hpp for tests/test_knn2_wide_dispatch.py: the choices inside Knn2Form::mfma.  One line per argument:
//   wide:nq_cap:nt_cap:batch:wide_env     1 / 0   knn2_mfma_wide (wide_env: -1 = SNK_BF_MFMA_WIDE unset, 0 / 1 = forced)
//   short:nt_cap:allowed                  1 / 0   knn2_mfma_short
//   knn2:nq_cap:nt_cap:batch:no_mfma      the form's name, as tests/cpp/dispatch_driver.cpp prints it
//   const:NAME
// Exit status 2 on an argument it cannot read.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "dispatch.hpp"

// the bench batch takes the wide form with 13-bit keys, one frame per call the narrow one: part of the header's contract
static_assert(snk::knn2_mfma_wide(1000, 1000, 1024, -1) && !snk::knn2_mfma_wide(1000, 1000, 1, -1), "knn2_mfma_wide");
static_assert(snk::knn2_mfma_short(1000, true) && !snk::knn2_mfma_short(1000, false), "knn2_mfma_short");

int main(int argc, char** argv)
{
    for (int a = 1; a < argc; ++a)
    {
        std::vector<std::string> f;
        std::string s(argv[a]);
        size_t p = 0, q;
        while ((q = s.find(':', p)) != std::string::npos) f.push_back(s.substr(p, q - p)), p = q + 1;
        f.push_back(s.substr(p));
        std::vector<long long> v;
        if (f[0] != "const")
            for (size_t i = 1; i < f.size(); ++i) v.push_back(std::atoll(f[i].c_str()));
        if (f[0] == "wide" && v.size() == 4) std::printf("%d\n", snk::knn2_mfma_wide((int)v[0], (int)v[1], (int)v[2], (int)v[3]) ? 1 : 0);
        else if (f[0] == "short" && v.size() == 2) std::printf("%d\n", snk::knn2_mfma_short((int)v[0], v[1] != 0) ? 1 : 0);
        else if (f[0] == "knn2" && v.size() == 4)
        {
            const snk::Knn2Form k = snk::knn2_form((int)v[0], (int)v[1], (int)v[2], v[3] != 0);
            std::printf("%s\n", k == snk::Knn2Form::mfma ? "mfma" : k == snk::Knn2Form::vector4 ? "vector4" : "vector1");
        }
        else if (f[0] == "const" && f.size() == 2 && f[1] == "BF_MFMA_WIDE_MIN_WGS") std::printf("%d\n", snk::BF_MFMA_WIDE_MIN_WGS);
        else if (f[0] == "const" && f.size() == 2 && f[1] == "BF_MFMA_SHORT_NT") std::printf("%d\n", snk::BF_MFMA_SHORT_NT);
        else
        {
            std::fprintf(stderr, "knn2_wide_driver: cannot read %s\n", argv[a]);
            return 2;
        }
    }
    return 0;
}
