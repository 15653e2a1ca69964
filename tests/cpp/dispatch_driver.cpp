// CPU build of dispatch.hpp (tests/test_cpp_dispatch.py): prints, one line per argument, the kernel form (or the LDS carve, or the
// constant) that the library's dispatch rules give for a launch shape.  An argument is "entry:a:b:..." with the integer arguments of
// the function of that name in dispatch.hpp, switches as 0 / 1:
//   knn2:nq_cap:nt_cap:batch:no_mfma              stereo_host:nr:sort_network
//   stereo_batch:nr_cap:batch:no_frame_kernel:sort_network
//   pose_host:total:n_problems:no_lds             pose_host_carve:n_max:n_problems
//   pose_batch:stride:batch:n_cu:waves_env:no_lds pose_batch_carve:stride:batch:lds_env:two_waves
//   ba_lm:<shape>:recording:switches              the five forms of an LM iteration, "lin/cam/schur/pcg/update"
//   ba_lm_nums:<shape>:recording:switches         "use_set,nsx,nbs,nbx,pcg_lds,zero_rows,split_copy,no_block_lists,chains"
//   ba_plain:<shape>:iterations:switches          1: snk_ba_solve_async issues plain launches whatever the history
//     <shape> = count:implicit:n6:nfc:np:ni:wv:rpc:items:set_ok:set_small:k:run:wave_ok:sums_ok:blk:pwgs:pone:prows (BaShape)
//     switches = comma-separated NAME=VALUE, the names of BaSwitches' comments (SNK_BA_ left off; DEBUG), or empty
//   ba_pcg_large:n6:nfc:implicit                  ba_chains:count:recording:pcg_large:chains_env
//   ba_reg_rows:n6:switches                       ba_sets:<shape>:switches
//   ba_persist:count:n6:nfc:coop:n_cu:res_persist:res_persist1:res_reg:switches    "wgs,one,rows"
//   ba_persist_imp:np:nfc:coop:n_cu:res:switches                                    "wgs,one,rows"
//   orb_band:n_strips:h:batch:bh_env              orb_cpw:total_cells:batch:cpw_env (the number)
//   orb_fast:quads:cpw                            orb_harris:total_cells:harris:per_cell
//   orb_dist:n_levels:batch:level_cap:harris      orb_desc:switches
//   orb_xcd:gx:batch                              "x,y"
//   orb_sched:batch:parts:stagger:split_min_batch:one_stream     orb_sched_n:... (chains, or parts of the staggered schedule)
//   orb_geom:<config>:switches                    per level "w,h,scale,nfeat,pitch,strip_stride,n_strips,store_end,n_bands,ncols,nrows,wcell,hcell,slot_cap,nroots", joined by ';'
//   orb_slice:<config>:switches                   "tile_pitch_dw,s_pitch,off_s,off_surv,off_list,off_cnt,lds_wave,surv_cap,quads,cells,slots,units,list_fits,fast_fits"
//   orb_plan:<config>:batch:aligned0:harris:stages:switches      "levels;cpw/quads;harris;dist;desc" as run_part's plan line names them
//   orb_plan_nums:...                             "fast_gx,fast_lds,harris_gx,lds_cap,dist_lds,large_workers,queue_memset,desc_gx,desc_nb,dfake,blur_mode;n_bands.gx per level"
//     <config> = w:h:nfeatures:n_levels:scale_factor:level_cap;  switches: as above with the names of OrbSwitches' comments (SNK_ORB_ left off)
//   track_form:pts_cap:batch:cap:ncell1:no_frame_lds:ppw_env     track_plan:pts_cap:batch:cap:ncell1:no_frame_lds:frame_wgs:no_fused_resolve:ppw_env  "ppw,wgs,claim_off,lds"
//   track_wgs:chunks:batch:forced                 track_claim:wgs:frame_lds:cap:off
//   track_ppw:total_points:ppw_env                track_lds:cap:ncell1
//   track_launch:pts_cap:batch:cap:ncell1:no_frame_lds:frame_wgs:no_fused_resolve:ppw_env    "form/wgs/resolve" as the plan line of a batched matcher names them
//   track_resolve_lds:cap                         1: the separate resolution keeps its claims in LDS
//   grid_form:cap:ncell:network_env               grid_lds:n:ncell (the counting form's LDS)
//   capacity:bytes                                what a scratch buffer asked for that many bytes holds
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

// "NO_POINT_WAVE=1,SCHUR_SET_MIN_ITEMS=1" -> BaSwitches, by the rules of ba_switches() in ba.hip: a flag is on when it is named
static bool read_switches(const std::string& list, snk::BaSwitches& s)
{
    size_t p = 0;
    while (p < list.size())
    {
        size_t q = list.find(',', p);
        if (q == std::string::npos) q = list.size();
        const std::string item = list.substr(p, q - p);
        p                      = q + 1;
        const size_t eq        = item.find('=');
        const std::string k    = item.substr(0, eq);
        const long long v      = eq == std::string::npos ? 1 : std::atoll(item.c_str() + eq + 1);
        const int pos          = v > 0 ? (int)v : 0;
        if (k == "PCG_GENERAL") s.pcg_general = true;
        else if (k == "NO_POINT_WAVE") s.no_point_wave = true;
        else if (k == "NO_SCHUR_SET") s.no_schur_set = true;
        else if (k == "SCHUR_SET_MIN_ITEMS") s.set_min_items = v;
        else if (k == "NO_SCHUR_MFMA") s.no_schur_mfma = true;
        else if (k == "NO_SCHUR_FUSED") s.no_schur_fused = true;
        else if (k == "FUSED_K10") s.fused_k10 = true;
        else if (k == "CAM_SUMS") s.cam_sums = true;
        else if (k == "CAM_GRID_2D") s.cam_grid_2d = true;
        else if (k == "NO_SCHUR_WIDE") s.no_schur_wide = true;
        else if (k == "PCG_LDS") s.pcg_lds = true;
        else if (k == "NO_UPDATE_COST") s.no_update_cost = true;
        else if (k == "FLAT_BARRIER") s.flat_barrier = true;
        else if (k == "PCG_TIMING") s.pcg_timing = true;
        else if (k == "PCGL_LAUNCHES") s.pcgl_launches = true;
        else if (k == "PERSIST_TWO_BARRIERS") s.persist_two_barriers = true;
        else if (k == "PERSIST_STREAM") s.persist_stream = true;
        else if (k == "PERSIST_WGS") s.persist_wgs = pos;
        else if (k == "PERSIST_REG_ROWS") s.persist_reg_rows = pos;
        else if (k == "PERSIST_FAIL") s.persist_fail = true;
        else if (k == "GRAPH_CHAINS") s.graph_chains = pos;
        else if (k == "NO_GRAPH") s.no_graph = true;
        else if (k == "GRAPH_FIRST") s.graph_first = true;
        else if (k == "LOCAL_SYNC") s.local_sync = true;
        else if (k == "DEBUG") s.debug = true;
        else return false;
    }
    return true;
}

// "LEVEL_BH=22,UNFUSED" -> OrbSwitches, by the rules of orb_switches() in orb.hip
static bool read_orb_switches(const std::string& list, snk::OrbSwitches& s)
{
    size_t p = 0;
    while (p < list.size())
    {
        size_t q = list.find(',', p);
        if (q == std::string::npos) q = list.size();
        const std::string item = list.substr(p, q - p);
        p                      = q + 1;
        const size_t eq        = item.find('=');
        const std::string name = item.substr(0, eq);
        const long long v      = eq == std::string::npos ? 0 : std::atoll(item.c_str() + eq + 1);
        const auto is          = [&](const char* n) { return name == n; };
        if (is("BALANCED_STRIPS")) s.balanced_strips = true;
        else if (is("FAST_SURV_CAP")) s.fast_surv_cap = v < 128 ? 128 : (int)v;
        else if (is("PARTS")) s.parts = v < 1 ? 1 : v > 4 ? 4 : (int)v;
        else if (is("STAGGER")) s.stagger = v >= 2 ? (v > 16 ? 16 : (int)v) : 0;
        else if (is("BLUR_IN_DESCRIBE")) s.blur_in_describe = true;
        else if (is("BLUR_TILED")) s.blur_tiled = true;
        else if (is("DESC_NO_DMA")) s.desc_no_dma = true;
        else if (is("DESC_FAKE")) s.desc_fake_on = true, s.desc_fake = (int)v;
        else if (is("UNFUSED")) s.unfused = true;
        else if (is("LEVEL_BH")) s.level_bh = (int)v;
        else if (is("FAST_CPW")) s.fast_cpw = (int)v;
        else if (is("FAST_STOP")) s.fast_stop = (int)v;
        else if (is("FAST_LDS_WG")) s.fast_lds_wg = (size_t)v;
        else if (is("DIST_TIMING")) s.dist_timing = true;
        else if (is("DIST_KEY_LOOP")) s.dist_key_loop = true;
        else if (is("HARRIS_PER_CELL")) s.harris_per_cell = true;
        else if (is("ONE_STREAM")) s.one_stream = true;
        else return false;
    }
    return true;
}

// orb_geom / orb_slice / orb_plan / orb_plan_nums: the fields "w:h:nfeatures:n_levels:scale_factor:level_cap" in front
constexpr size_t ORB_CONFIG_ARGS = 6;
static const char* orb_layout_of(const std::vector<std::string>& f, const snk::OrbSwitches& sw, snk::Layout& L)
{
    return snk::orb::layout(L, std::atoi(f[1].c_str()), std::atoi(f[2].c_str()), std::atoi(f[3].c_str()), (float)std::atof(f[5].c_str()), std::atoi(f[4].c_str()),
                            std::atoi(f[6].c_str()), sw.balanced_strips, sw.fast_surv_cap);
}

static int orb_entry(const std::string& e, const std::vector<std::string>& f, const snk::OrbSwitches& sw)
{
    snk::Layout L;
    const char* bad = orb_layout_of(f, sw, L);
    if (e == "orb_geom")
    {
        for (int l = 0; l < L.n_levels; ++l)
        {
            const snk::LevelInfo& v = L.lv[l];
            std::printf("%s%d,%d,%.9g,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d", l ? ";" : "", v.w, v.h, (double)v.scale, v.nfeat, v.pitch, v.strip_stride, v.n_strips, v.store_end,
                        v.n_bands, v.ncols, v.nrows, v.wcell, v.hcell, v.slot_cap, v.nroots);
        }
        std::printf("\n");
    }
    else if (e == "orb_slice")
        std::printf("%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d\n", L.f_tile_pitch_dw, L.f_s_pitch, L.f_off_s, L.f_off_surv, L.f_off_list, L.f_off_cnt, L.f_lds_wave,
                    L.f_surv_cap, snk::orb::fast_quads(L), L.total_cells, L.total_slots, L.total_units, (int)(bad == nullptr), (int)snk::orb::fast_fits(L));
    else
    {
        const size_t a        = ORB_CONFIG_ARGS + 1;
        const snk::OrbPlan P  = snk::orb_plan(L, std::atoi(f[a].c_str()), std::atoi(f[a + 1].c_str()) != 0, std::atoi(f[a + 2].c_str()) != 0, std::atoi(f[a + 3].c_str()),
                                              (float)std::atof(f[5].c_str()), sw);
        if (e == "orb_plan")
        {
            for (int l = 0; l < P.n_levels; ++l)
            {
                char tok[8];
                snk::orb_level_token(P.lv[l], tok);
                std::printf("%s%s", l ? "," : "", tok);
            }
            std::printf(";%d/%d;%s;%s;%s\n", P.fast_run ? P.fast_cpw : 0, P.fast_quads, snk::orb_name(P.harris), snk::orb_name(P.dist), snk::orb_name(P.desc));
        }
        else
        {
            std::printf("%d,%zu,%d,%d,%zu,%d,%d,%d,%d,%d,%d", P.fast_gx, P.fast_lds, P.harris_gx, P.dist_lds_cap, P.dist_lds, P.large_workers, (int)P.queue_memset, P.desc_gx,
                        P.desc_nb, P.dfake, P.blur_mode);
            for (int l = 0; l < P.n_levels; ++l) std::printf("%s%d.%d", l ? "," : ";", P.lv[l].n_bands, P.lv[l].gx);
            std::printf("\n");
        }
    }
    return 0;
}

constexpr size_t BA_SHAPE_ARGS = 19;
static snk::BaShape read_shape(const std::vector<long long>& v)
{
    snk::BaShape s;
    s.count = (int)v[0], s.implicit = v[1] != 0, s.max_n6 = (int)v[2], s.max_nfc = (int)v[3], s.max_np = (int)v[4], s.max_ni = (int)v[5];
    s.max_wv = (int)v[6], s.max_rpc = (int)v[7], s.max_set_items = (int)v[8], s.set_ok = v[9] != 0, s.set_small = v[10] != 0;
    s.set_k_max = (int)v[11], s.set_run_max = (int)v[12], s.point_wave_ok = v[13] != 0, s.cam_sums_ok = v[14] != 0, s.blk_built = v[15] != 0;
    s.persist_wgs = (int)v[16], s.persist_one = (int)v[17], s.persist_rows = (int)v[18];
    return s;
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
        snk::BaSwitches sw;
        const bool ba = e.compare(0, 3, "ba_") == 0 && e != "ba_pcg_large" && e != "ba_chains";  // the last field: the switches
        if (ba && (f.size() < 2 || !read_switches(f.back(), sw)))
        {
            std::fprintf(stderr, "dispatch_driver: cannot read the switches of %s\n", argv[a]);
            return 2;
        }
        const bool orb_sw = e == "orb_desc" || e == "orb_geom" || e == "orb_slice" || e == "orb_plan" || e == "orb_plan_nums";  // the last field: the switches
        snk::OrbSwitches osw;
        if (orb_sw)
        {
            const size_t want = e == "orb_desc" ? 2 : ORB_CONFIG_ARGS + 2 + (e == "orb_plan" || e == "orb_plan_nums" ? 4 : 0);
            if (f.size() != want || !read_orb_switches(f.back(), osw))
            {
                std::fprintf(stderr, "dispatch_driver: cannot read %s\n", argv[a]);
                return 2;
            }
            if (e == "orb_desc") std::printf("%s\n", snk::orb_name(snk::orb_desc_form(osw)));
            else orb_entry(e, f, osw);
            continue;
        }
        if (e != "const")
            for (size_t i = 1; i + (ba ? 1 : 0) < f.size(); ++i) v.push_back(std::atoll(f[i].c_str()));
        const size_t n = v.size();
        if (e == "ba_lm" && n == BA_SHAPE_ARGS + 1)
        {
            const snk::BaLmPlan P = snk::ba_lm_plan(read_shape(v), sw, v[BA_SHAPE_ARGS] != 0);
            std::printf("%s/%s/%s/%s/%s\n", snk::ba_name(P.lin), snk::ba_name(P.cam), snk::ba_name(P.schur), snk::ba_name(P.pcg), snk::ba_name(P.update));
        }
        else if (e == "ba_lm_nums" && n == BA_SHAPE_ARGS + 1)
        {
            const snk::BaLmPlan P = snk::ba_lm_plan(read_shape(v), sw, v[BA_SHAPE_ARGS] != 0);
            std::printf("%d,%d,%d,%d,%zu,%d,%d,%d,%d\n", (int)P.use_set, P.nsx, P.nbs, P.nbx, P.pcg_lds, (int)P.zero_rows, (int)P.split_copy,
                        (int)P.no_block_lists, P.n_chain);
        }
        else if (e == "ba_plain" && n == BA_SHAPE_ARGS + 1) std::printf("%d\n", (int)snk::ba_solve_plain(read_shape(v), sw, (int)v[BA_SHAPE_ARGS]));
        else if (e == "ba_sets" && n == BA_SHAPE_ARGS) std::printf("%d\n", (int)snk::ba_sets_will_run(read_shape(v), sw));
        else if (e == "ba_pcg_large" && n == 3) std::printf("%d\n", (int)snk::ba_pcg_is_large((int)v[0], (int)v[1], v[2] != 0));
        else if (e == "ba_chains" && n == 4) std::printf("%d\n", snk::ba_graph_chains((int)v[0], v[1] != 0, v[2] != 0, (int)v[3]));
        else if (e == "ba_reg_rows" && n == 1) std::printf("%d\n", snk::ba_persist_reg_rows((int)v[0], sw));
        else if (e == "ba_persist" && n == 8)
        {
            const snk::BaPersist P = snk::ba_persist_dense((int)v[0], (int)v[1], (int)v[2], v[3] != 0, (int)v[4], (int)v[5], (int)v[6], (int)v[7], sw);
            std::printf("%d,%d,%d\n", P.wgs, P.one, P.rows);
        }
        else if (e == "ba_persist_imp" && n == 5)
        {
            const snk::BaPersist P = snk::ba_persist_implicit((int)v[0], (int)v[1], v[2] != 0, (int)v[3], (int)v[4], sw);
            std::printf("%d,%d,%d\n", P.wgs, P.one, P.rows);
        }
        else if (e == "knn2" && n == 4) std::printf("%s\n", name(snk::knn2_form((int)v[0], (int)v[1], (int)v[2], v[3] != 0)));
        else if (e == "stereo_host" && n == 2) std::printf("%s\n", name(snk::stereo_host_form((int)v[0], v[1] != 0)));
        else if (e == "stereo_batch" && n == 4) std::printf("%s\n", name(snk::stereo_batch_form((int)v[0], (int)v[1], v[2] != 0, v[3] != 0)));
        else if (e == "pose_host" && n == 3) std::printf("%s\n", name(snk::pose_host_form((size_t)v[0], (int)v[1], v[2] != 0)));
        else if (e == "pose_host_carve" && n == 2) std::printf("%d\n", snk::pose_host_carve((int)v[0], (int)v[1]));
        else if (e == "pose_batch" && n == 5) std::printf("%s\n", name(snk::pose_batch_form((int)v[0], (int)v[1], (int)v[2], (int)v[3], v[4] != 0)));
        else if (e == "pose_batch_carve" && n == 4) std::printf("%d\n", snk::pose_batch_carve((int)v[0], (int)v[1], (int)v[2], v[3] != 0));
        else if (e == "orb_band" && n == 4) std::printf("%s\n", snk::orb_name(snk::orb_band_form((int)v[0], (int)v[1], (int)v[2], (int)v[3])));
        else if (e == "orb_cpw" && n == 3) std::printf("%d\n", snk::orb_fast_cpw((int)v[0], (int)v[1], (int)v[2]));
        else if (e == "orb_fast" && n == 2) std::printf("%s\n", snk::orb_name(snk::orb_fast_form((int)v[0], v[1] > 1)));
        else if (e == "orb_harris" && n == 3) std::printf("%s\n", snk::orb_name(snk::orb_harris_form((int)v[0], v[1] != 0, v[2] != 0)));
        else if (e == "orb_dist" && n == 4) std::printf("%s\n", snk::orb_name(snk::orb_dist_form((int)v[0], (int)v[1], (int)v[2], v[3] != 0)));
        else if (e == "orb_xcd" && n == 2)
        {
            int x, y;
            snk::orb_xcd_grid((int)v[0], (int)v[1], x, y);
            std::printf("%d,%d\n", x, y);
        }
        else if ((e == "orb_sched" || e == "orb_sched_n") && n == 5)
        {
            int parts;
            const snk::OrbSchedule sc = snk::orb_schedule((int)v[0], (int)v[1], (int)v[2], (int)v[3], v[4] != 0, parts);
            if (e == "orb_sched") std::printf("%s\n", snk::orb_name(sc));
            else std::printf("%d\n", parts);
        }
        else if ((e == "track_form" && n == 6) || (e == "track_plan" && n == 8))
        {
            snk::TrackSwitches ts;
            ts.no_frame_lds = v[4] != 0;
            if (e == "track_form") ts.ppw = (int)v[5];
            else ts.frame_wgs = (int)v[5], ts.no_fused_resolve = v[6] != 0, ts.ppw = (int)v[7];
            const snk::TrackBatchPlan P = snk::track_batch_plan((int)v[0], (int)v[1], (int)v[2], (int)v[3], ts);
            if (e == "track_form") std::printf("%s\n", snk::track_name(P.form));
            else std::printf("%d,%d,%d,%zu\n", P.ppw, P.wgs, P.claim_off, P.lds);
        }
        else if (e == "track_launch" && n == 8)
        {
            snk::TrackSwitches ts;
            ts.no_frame_lds = v[4] != 0, ts.frame_wgs = (int)v[5], ts.no_fused_resolve = v[6] != 0, ts.ppw = (int)v[7];
            const snk::TrackBatchPlan P = snk::track_batch_plan((int)v[0], (int)v[1], (int)v[2], (int)v[3], ts);
            std::printf("%s/%d/%s\n", snk::track_name(P.form), P.wgs, snk::track_name(snk::track_resolve_form(P, (int)v[2])));
        }
        else if (e == "track_resolve_lds" && n == 1) std::printf("%d\n", (int)snk::track_resolve_in_lds((int)v[0]));
        else if (e == "grid_form" && n == 3) std::printf("%s\n", snk::grid_name(snk::grid_form((int)v[0], (int)v[1], v[2] != 0)));
        else if (e == "grid_lds" && n == 2) std::printf("%zu\n", snk::grid_count_lds((int)v[0], (int)v[1]));
        else if (e == "track_wgs" && n == 3) std::printf("%d\n", snk::track_frame_wgs((int)v[0], (int)v[1], (int)v[2]));
        else if (e == "track_claim" && n == 4) std::printf("%d\n", snk::track_fused_claim_offset((int)v[0], (size_t)v[1], (int)v[2], v[3] != 0));
        else if (e == "track_ppw" && n == 2) std::printf("%d\n", snk::track_points_per_wave(v[0], (int)v[1]));
        else if (e == "track_lds" && n == 2) std::printf("%zu\n", snk::track_frame_lds((int)v[0], (int)v[1]));
        else if (e == "capacity" && n == 1) std::printf("%zu\n", snk::scratch_capacity((size_t)v[0]));
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
            else if (c == "BA_SET_MIN_ITEMS") val = snk::BA_SET_MIN_ITEMS;
            else if (c == "BA_FUSED3_MAX_K") val = snk::BA_FUSED3_MAX_K;
            else if (c == "BA_CAM64_MIN_BATCH") val = snk::BA_CAM64_MIN_BATCH;
            else if (c == "BA_SCHUR_WIDE_BATCH_END") val = snk::BA_SCHUR_WIDE_BATCH_END;
            else if (c == "BA_SCHUR_WIDE_MAX_BLOCKS") val = snk::BA_SCHUR_WIDE_MAX_BLOCKS;
            else if (c == "BA_PCG_SMALL_MAX_N6") val = snk::BA_PCG_SMALL_MAX_N6;
            else if (c == "BA_PCG_LDS_MAX") val = snk::BA_PCG_LDS_MAX;
            else if (c == "BA_PERSIST_LDS_MAX") val = snk::BA_PERSIST_LDS_MAX;
            else if (c == "PREG_MAX_N6") val = snk::PREG_MAX_N6;
            else if (c == "BA_PREG_ROWS16_ABOVE_N6") val = snk::BA_PREG_ROWS16_ABOVE_N6;
            else if (c == "BA_SPLIT_COPY_MAX_BATCH") val = snk::BA_SPLIT_COPY_MAX_BATCH;
            else if (c == "BA_SPLIT_COPY_MIN_POINTS") val = snk::BA_SPLIT_COPY_MIN_POINTS;
            else if (c == "BA_GRAPH_CHAINS") val = snk::BA_GRAPH_CHAINS;
            else if (c == "BA_GRAPH_CHAINS_MIN_BATCH") val = snk::BA_GRAPH_CHAINS_MIN_BATCH;
            else if (c == "BA_GRAPH_CHAIN_MIN") val = snk::BA_GRAPH_CHAIN_MIN;
            else if (c == "SUM_NB") val = snk::SUM_NB;
            else if (c == "PERSIST_WGS_MAX") val = snk::PERSIST_WGS_MAX;
            else if (c == "ORB_BAND_MIN_WAVES") val = snk::ORB_BAND_MIN_WAVES;
            else if (c == "ORB_WAVE_SLOTS") val = snk::ORB_WAVE_SLOTS;
            else if (c == "ORB_FAST_CPW_DEFAULT") val = snk::ORB_FAST_CPW_DEFAULT;
            else if (c == "ORB_FAST_MIN_ROUNDS") val = snk::ORB_FAST_MIN_ROUNDS;
            else if (c == "ORB_XCD_MIN_BATCH") val = snk::ORB_XCD_MIN_BATCH;
            else if (c == "ORB_DIST_ONE_MAX_WGS") val = snk::ORB_DIST_ONE_MAX_WGS;
            else if (c == "ORB_DIST_LARGE_WGS") val = snk::ORB_DIST_LARGE_WGS;
            else if (c == "ORB_DIST_SMALL_CAP") val = snk::orb::DIST_SMALL_CAP;
            else if (c == "ORB_DIST_LDS_MAX") val = (int)snk::orb::DIST_LDS_MAX;
            else if (c == "ORB_DIST_LARGE_LDS_MAX") val = (int)snk::orb::DIST_LARGE_LDS_MAX;
            else if (c == "TRACK_FRAME_LDS_MAX") val = snk::TRACK_FRAME_LDS_MAX;
            else if (c == "TRACK_PPW_POINTS") val = snk::TRACK_PPW_POINTS;
            else if (c == "TRACK_CHUNK_POINTS") val = snk::TRACK_CHUNK_POINTS;
            else if (c == "TRACK_RESOLVE_LDS_FEATURES") val = snk::TRACK_RESOLVE_LDS_FEATURES;
            else if (c == "GRID_MAX_FEATURES") val = snk::GRID_MAX_FEATURES;
            else if (c == "GRID_COUNT_LDS_MAX") val = snk::GRID_COUNT_LDS_MAX;
            else if (c == "MATCHER_SCRATCH_BYTES") val = (int)snk::MATCHER_SCRATCH_BYTES;
            else if (c == "MATCHER_H_IN_BYTES") val = (int)snk::MATCHER_H_IN_BYTES;
            else if (c == "MATCHER_H_RES_BYTES") val = (int)snk::MATCHER_H_RES_BYTES;
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
