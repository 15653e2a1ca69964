// CPU build of dispatch.hpp (tests/test_cpp_dispatch.py): prints, one line per argument, the kernel form (or the LDS carve, or the
// constant) that the library's dispatch rules give for a launch shape.  An argument is "entry:a:b:..." with the integer arguments of
// the function of that name in dispatch.hpp, switches as 0 / 1:
//   knn2:nq_cap:nt_cap:batch:no_mfma              stereo_host:nr:sort_network
//   stereo_batch:nr_cap:batch:no_frame_kernel:sort_network
//   pose_host:total:n_problems:no_lds             pose_host_carve:n_max:n_problems
//   pose_batch:stride:batch:n_cu:waves_env:no_lds pose_batch_carve:stride:batch:lds_env:two_waves
//   const:NAME
// Exit status 2 on an argument it cannot read.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "dispatch.hpp"

static const char* name(snk::Knn2Form f)
{
    switch (f)
    {
    case snk::Knn2Form::vector1: return "vector1";
    case snk::Knn2Form::vector4: return "vector4";
    case snk::Knn2Form::mfma: return "mfma";
    }
    return "?";
}
static const char* name(snk::StereoForm f)
{
    switch (f)
    {
    case snk::StereoForm::frame: return "frame";
    case snk::StereoForm::count16: return "count16";
    case snk::StereoForm::sort16: return "sort16";
    case snk::StereoForm::unindexed: return "unindexed";
    }
    return "?";
}
static const char* name(snk::PoseForm f)
{
    switch (f)
    {
    case snk::PoseForm::wave1: return "wave1";
    case snk::PoseForm::wave2_lds: return "wave2_lds";
    case snk::PoseForm::wave4_lds: return "wave4_lds";
    case snk::PoseForm::wave4_global: return "wave4_global";
    }
    return "?";
}

int main(int argc, char** argv)
{
    for (int a = 1; a < argc; ++a)
    {
        std::vector<std::string> f;
        {
            std::string s(argv[a]);
            size_t p = 0, q;
            while ((q = s.find(':', p)) != std::string::npos) f.push_back(s.substr(p, q - p)), p = q + 1;
            f.push_back(s.substr(p));
        }
        const std::string& e = f[0];
        std::vector<long long> v;
        if (e != "const")
            for (size_t i = 1; i < f.size(); ++i) v.push_back(std::atoll(f[i].c_str()));
        const size_t n = v.size();
        if (e == "knn2" && n == 4) std::printf("%s\n", name(snk::knn2_form((int)v[0], (int)v[1], (int)v[2], v[3] != 0)));
        else if (e == "stereo_host" && n == 2) std::printf("%s\n", name(snk::stereo_host_form((int)v[0], v[1] != 0)));
        else if (e == "stereo_batch" && n == 4) std::printf("%s\n", name(snk::stereo_batch_form((int)v[0], (int)v[1], v[2] != 0, v[3] != 0)));
        else if (e == "pose_host" && n == 3) std::printf("%s\n", name(snk::pose_host_form((size_t)v[0], (int)v[1], v[2] != 0)));
        else if (e == "pose_host_carve" && n == 2) std::printf("%d\n", snk::pose_host_carve((int)v[0], (int)v[1]));
        else if (e == "pose_batch" && n == 5) std::printf("%s\n", name(snk::pose_batch_form((int)v[0], (int)v[1], (int)v[2], (int)v[3], v[4] != 0)));
        else if (e == "pose_batch_carve" && n == 4) std::printf("%d\n", snk::pose_batch_carve((int)v[0], (int)v[1], (int)v[2], v[3] != 0));
        else if (e == "const" && f.size() == 2)
        {
            const std::string& c = f[1];
            int val;
            if (c == "ST_SORT_MAX") val = snk::ST_SORT_MAX;
            else if (c == "ST_FRAME_MAX") val = snk::ST_FRAME_MAX;
            else if (c == "ST_FRAME_BATCH") val = snk::ST_FRAME_BATCH;
            else if (c == "ST_COUNT_ROWS") val = snk::ST_COUNT_ROWS;
            else if (c == "BF_MFMA_MIN") val = snk::BF_MFMA_MIN;
            else if (c == "BF_WIDE_MIN_WORK") val = snk::BF_WIDE_MIN_WORK;
            else if (c == "POSE_HOST_WAVE4_MEAN") val = snk::POSE_HOST_WAVE4_MEAN;
            else if (c == "POSE_BATCH_WAVE4_MIN") val = snk::POSE_BATCH_WAVE4_MIN;
            else if (c == "POSE_SLOTS_PER_WAVE") val = snk::POSE_SLOTS_PER_WAVE;
            else
            {
                std::fprintf(stderr, "dispatch_driver: no constant %s\n", c.c_str());
                return 2;
            }
            std::printf("%d\n", val);
        }
        else
        {
            std::fprintf(stderr, "dispatch_driver: cannot read %s\n", argv[a]);
            return 2;
        }
    }
    return 0;
}
