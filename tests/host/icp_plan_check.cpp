// Stand-alone check of the ICP launcher's plan (sonar_slam_amd/csrc/sfe_icp_sweep_plan.h), run on the CPU.
// tests/test_icp_plan_rules.py builds it plainly; under the sanitizers it is a program of its own (no GPU, nothing
// preloaded):
//   g++ -std=c++17 -O1 -g -Wall -Wextra -Werror -fsanitize=address,undefined -fno-sanitize-recover=all
//       tests/host/icp_plan_check.cpp -o icp_plan_check && ./icp_plan_check [CALLS.txt]
//
// CALLS.txt (written by the test from tests/golden/icp_routes.json): one call per line with the route of every job and
// the launches that the kernel trace of the commit before this header showed for it.  The plan must give the same routes
// and, launch by launch, the same kernel, template arguments, workgroups and workgroup size.  (The trace's LDS figure is
// the kernels' static LDS alone -- none for the loop kernel, whose whole layout is dynamic; it is compared with those
// constants.)  The calls named q_*_fits / q_*_over must sit on the two sides of the fit that the header's constants
// give, and each job of odd_mix must take the Q class when it is planned alone.
//
// Without a file, and before it: the invariants the executor and the kernels rely on, over a grid of
//   job lists   one shape x {1, n_cu, n_cu + 1, 2 n_cu - 1, 2 n_cu, 2 n_cu + 3} jobs for each of 22 shapes at the tiers'
//               edges, and (n_cu 4 and 256; flags none, profile and the last) every pair of 11 of them x {1, 2 n_cu}
//               jobs each; the jobs of a group on one target or on one target each;
//   chains      point-to-point and point-to-plane (normals_knn 8, 10, 12, 16); the shipped checker, 30 and 11 fixed
//               iterations;
//   tuning      default; sw_tiers = sw_tiny = 0; sw_tiny = 0; sw_multi = 0; sw_multi_g = 4 with sw_multi_min_src = 1000,
//               sw_multi_share_min = 100; sw_rec = 0;
//   flags       none; profile; outlier modules; sfe_icp_set_tuning bit 4; unsplit; side stream + profile + outliers;
//   n_cu        1, 4, 256, 304.
//   * every caller's job has one route, and its record(s) are in that class's list and in no other; the id lists
//     partition the job records; the launches take the lists one after the other, in the table's order;
//   * the shares of a split job are contiguous records, shares 0 .. ngrp - 1 of one sync area; all shares together
//     fit the CUs (shares x big jobs <= n_cu); no job is split under bit 4, unsplit or sw_multi = 0;
//   * t_cap / q_cap of every launch cover its jobs, `body` is the layout's size, and control block + body fit the LDS
//     share the plan assumed (160 KiB for the small tiers) -- the control block without the profile's counters: with
//     the profile on, two jobs of 1405 x 8192 on one CU take 624 bytes more than the 80 KiB share; every launch fits
//     the CU's 160 KiB;
//   * the 1024-thread launches take the 128-VGPR builds exactly when `wide`;
//   * the q_off slices of the caller's jobs are disjoint and inside qoff, the targets' slices inside toff / koff /
//     goff, grid offsets multiples of 64;
//   * the struct tables start 16-byte aligned, the id lists 4-byte aligned, all inside tab_bytes, and write_tables fills
//     exactly that block;
//   * a target that only tiny point-to-point jobs use is in no prep list, every other target in exactly one (its tier's);
//     pids_nrm = the point-to-plane targets beyond SW_TCAP;
//   * every build key is in SW_LOOP_BUILDS / SW_PREP_BUILDS, and every listed build is reached by some plan of the grid
//     (a build that no plan reaches is compile time spent for nothing).
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>

#include "../../sonar_slam_amd/csrc/sfe_icp_sweep_plan.h"

static const char *g_what = "";
static SweepPlanIn g_in;

#define CHECK(cond)                                                                                                    \
    do {                                                                                                               \
        if (!(cond)) {                                                                                                 \
            std::fprintf(stderr,                                                                                       \
                         "icp_plan_check: %s fails (line %d) %s: %d jobs (first %d x %d) minimizer %d max_iter %d diff %d " \
                         "knn %d tiers %d tiny %d multi %d g %d min_src %d share_min %d rec %d n_cu %d side %d no_split %d " \
                         "unsplit %d prof %d ox %d\n",                                                                 \
                         #cond, __LINE__, g_what, g_in.n_jobs, g_in.n_jobs ? g_in.jobs4[1] : 0, g_in.n_jobs ? g_in.jobs4[3] : 0, \
                         g_in.minimizer, g_in.max_iter, g_in.use_diff_checker, g_in.normals_knn, g_in.sw_tiers, g_in.sw_tiny, \
                         g_in.sw_multi, g_in.sw_multi_g, g_in.sw_multi_min_src, g_in.sw_multi_share_min, g_in.sw_rec,    \
                         g_in.n_cu, (int)g_in.side, (int)g_in.no_split, (int)g_in.unsplit, (int)g_in.prof, (int)g_in.ox); \
            std::exit(1);                                                                                              \
        }                                                                                                              \
    } while (0)

#define SW_X(...) SweepLoopBuild{__VA_ARGS__, false},
static const SweepLoopBuild LOOP_BUILDS[] = {SW_LOOP_BUILDS(SW_X)};
#undef SW_X
#define SW_X(...) SweepPrepBuild{__VA_ARGS__},
static const SweepPrepBuild PREP_BUILDS[] = {SW_PREP_BUILDS(SW_X)};
#undef SW_X
constexpr int N_LOOP = sizeof LOOP_BUILDS / sizeof *LOOP_BUILDS, N_PREP = sizeof PREP_BUILDS / sizeof *PREP_BUILDS;
static long long g_loop_hits[N_LOOP], g_prep_hits[N_PREP], g_class[SW_N_CLASSES], g_plans;

// the tuning defaults (sfe_tuning, sfe_internal.h; the test passes the file's own values for the fixture)
static SweepPlanIn defaults()
{
    SweepPlanIn in;
    in.sw_tiers = in.sw_tiny = in.sw_multi = in.sw_cache = in.sw_rec = 1;
    in.sw_multi_min_src = 8192, in.sw_multi_share_min = 1024, in.sw_strip_pts = 96;
    in.max_iter = 20, in.use_diff_checker = 1, in.normals_knn = 10, in.n_cu = 256;
    return in;
}

static const SweepPlan &checked_plan(const SweepPlanIn &in)
{
    static SweepPlan pl;
    static std::vector<int> seen_rec, per_out, prep_use;
    static std::vector<char> tables;
    g_in = in;
    sweep_plan(in, pl);
    ++g_plans;
    const int n_rec = (int)pl.jobs.size(), n_prep = (int)pl.preps.size();
    CHECK((int)pl.route.size() == in.n_jobs && n_rec >= in.n_jobs);
    // the id lists partition the records; a record sits in the list of its job's route
    seen_rec.assign((size_t)n_rec, 0);
    per_out.assign((size_t)in.n_jobs, 0);
    for (int c = 0; c < SW_N_CLASSES; ++c) {
        int last = -1;
        for (int r : pl.ids[c]) {
            CHECK(r >= 0 && r < n_rec && r > last && ++seen_rec[(size_t)r] == 1);
            last = r;
            const SweepJob &J = pl.jobs[(size_t)r];
            CHECK(J.out >= 0 && J.out < in.n_jobs && pl.route[(size_t)J.out] == c);
            ++per_out[(size_t)J.out];
            CHECK(J.ngrp >= 1 && J.grp >= 0 && J.grp < J.ngrp && (J.ngrp > 1) == (c == SFE_ICP_ROUTE_SPLIT));
            const int32_t *q = in.jobs4 + 4 * (size_t)J.out;
            CHECK(J.src_start == q[0] && J.n_src == q[1] && J.n_tgt == q[3] && J.prep >= 0 && J.prep < n_prep);
            const SweepPrep &P = pl.preps[(size_t)J.prep];
            CHECK(P.tgt_start == q[2] && P.n_tgt == q[3] && J.tgt_off == P.off);
        }
        g_class[c] += (long long)pl.ids[c].size();
    }
    for (int r = 0; r < n_rec; ++r)
        CHECK(seen_rec[(size_t)r] == 1);
    for (int j = 0; j < in.n_jobs; ++j)
        CHECK(per_out[(size_t)j] >= 1 && (per_out[(size_t)j] > 1) == (pl.route[(size_t)j] == SFE_ICP_ROUTE_SPLIT));
    // split jobs
    const bool may_split = in.sw_multi && !in.no_split && !in.unsplit;
    CHECK(may_split || pl.split_first.empty());
    CHECK((int)pl.split_first.size() == pl.n_sync && (int)pl.ids[SFE_ICP_ROUTE_SPLIT].size() <= (pl.n_sync ? in.n_cu : 0));
    CHECK(pl.n_sync == 0 || pl.wide);
    for (int s = 0; s < pl.n_sync; ++s) {
        const int r0 = pl.split_first[(size_t)s];
        CHECK(r0 >= 0 && r0 < n_rec);
        const SweepJob &J0 = pl.jobs[(size_t)r0];
        CHECK(J0.grp == 0 && J0.ngrp >= 2 && J0.ngrp <= SW_MG_MAX && J0.sync == s && r0 + J0.ngrp <= n_rec);
        CHECK((long long)J0.ngrp * pl.n_sync <= in.n_cu && J0.n_tgt > SW_TCAP && J0.n_src >= in.sw_multi_min_src);
        CHECK(per_out[(size_t)J0.out] == J0.ngrp);
        for (int g = 1; g < J0.ngrp; ++g) {
            const SweepJob &J = pl.jobs[(size_t)(r0 + g)];
            CHECK(J.out == J0.out && J.grp == g && J.ngrp == J0.ngrp && J.sync == s && J.q_off == J0.q_off);
        }
    }
    // the per-query slices of the caller's jobs: in the order of the records, one after the other
    long long q_end = 0;
    for (int r = 0; r < n_rec; ++r) {
        const SweepJob &J = pl.jobs[(size_t)r];
        if (J.grp == 0) {
            CHECK(J.q_off == q_end);
            q_end += J.n_src;
        }
    }
    CHECK(q_end == pl.qoff);
    // the targets' slices and the prep lists
    long long t_end = 0, k_end = 0, g_end = 0;
    seen_rec.assign((size_t)n_prep, 0);
    for (int t = 0; t < 3; ++t)
        for (int pid : pl.pids[t]) {
            CHECK(pid >= 0 && pid < n_prep && ++seen_rec[(size_t)pid] == 1 && pl.prep_tier[(size_t)pid] == t);
            CHECK(pl.preps[(size_t)pid].n_tgt <= (t == 0 ? SW_T0_TCAP : t == 1 ? SW_T1_TCAP : 1 << 24));
        }
    size_t n_nrm = 0;
    prep_use.assign((size_t)n_prep, 0); // 1: only tiny point-to-point jobs use the target, 2: another job does
    for (const SweepJob &J : pl.jobs)
        prep_use[(size_t)J.prep] |= (pl.route[(size_t)J.out] != SFE_ICP_ROUTE_TINY || in.minimizer == 1) ? 2 : 1;
    for (int pid = 0; pid < n_prep; ++pid) {
        const SweepPrep &P = pl.preps[(size_t)pid];
        CHECK(P.off == t_end && P.key_off == k_end && P.grid_off == g_end && P.grid_off % 64 == 0);
        CHECK(P.ns >= 1 && P.ns <= SW_NS_MAX);
        t_end += P.n_tgt + SW_PAD;
        CHECK(prep_use[(size_t)pid] != 0 && seen_rec[(size_t)pid] == (prep_use[(size_t)pid] == 1 ? 0 : 1));
        const bool nrm = P.n_tgt > SW_TCAP && in.minimizer == 1;
        CHECK(P.pad_ == (nrm ? 1 : 0));
        if (nrm) {
            CHECK(n_nrm < pl.pids_nrm.size() && pl.pids_nrm[n_nrm] == pid && pl.prep_tier[(size_t)pid] == 2);
            ++n_nrm;
        }
        if (P.n_tgt > SW_TCAP) { // a power of two of sort keys
            long long n2 = 2;
            while (n2 < P.n_tgt)
                n2 <<= 1;
            k_end += n2;
        }
        const int tier = pl.prep_tier[(size_t)pid];
        g_end += tier == 0 ? SW_T0_GRID : tier == 1 ? SW_T1_GRID : SW_GRID_MAX;
    }
    CHECK(n_nrm == pl.pids_nrm.size() && t_end == pl.toff && k_end == pl.koff && g_end == pl.goff);
    // the table block
    CHECK(pl.o_jobs % 16 == 0 && pl.o_ids % 16 == 0 && pl.o_split % 4 == 0 && pl.o_pids % 4 == 0 && pl.o_pnrm % 4 == 0);
    CHECK(pl.o_jobs >= sizeof(SweepPrep) * (size_t)n_prep && pl.o_ids >= pl.o_jobs + sizeof(SweepJob) * (size_t)n_rec);
    CHECK(pl.o_split == pl.o_ids + 4 * (size_t)n_rec && pl.o_pids == pl.o_split + 4 * pl.split_first.size());
    CHECK(pl.o_pnrm == pl.o_pids + 4 * (size_t)n_prep && pl.tab_bytes == pl.o_pnrm + 4 * pl.pids_nrm.size());
    tables.assign(pl.tab_bytes + 1, (char)0x5A);
    tables.shrink_to_fit(); // (a write past the block is the sanitizer's to see; the byte behind it is checked here)
    pl.write_tables(tables.data());
    CHECK(tables[pl.tab_bytes] == (char)0x5A);
    const int *t_ids = (const int *)(tables.data() + pl.o_ids);
    // the launches
    CHECK(pl.n_launches <= SW_MAX_LAUNCHES && pl.n_prep_launches <= pl.n_launches);
    int id_next = 0, pid_next = 0, cls = 0, kind_last = -1;
    const bool rec_chain = in.sw_rec && in.max_iter >= SW_REC_MIN_ITER && !in.use_diff_checker;
    CHECK(pl.rec_build == rec_chain);
    for (int i = 0; i < pl.n_launches; ++i) {
        const SweepLaunch &L = pl.launches[i];
        CHECK(L.n >= 1 && (int)L.kind >= kind_last && (i < pl.n_prep_launches) == (L.kind <= SW_LAUNCH_SPLIT));
        CHECK(L.kind == SW_LAUNCH_PREP || L.kind == SW_LAUNCH_LOOP || (int)L.kind > kind_last); // one normals / split / tiny launch
        kind_last = (int)L.kind;
        if (L.kind == SW_LAUNCH_PREP) {
            int b = 0;
            while (b < N_PREP && !sweep_same_build(L.prep, PREP_BUILDS[b]))
                ++b;
            CHECK(b < N_PREP);
            ++g_prep_hits[b];
            const int tier = L.prep.nt == SW_T0_NT ? 0 : L.prep.nt == SW_T1_NT ? 1 : 2;
            CHECK(L.id_off == pid_next && L.n == (int)pl.pids[tier].size());
            CHECK(tier < 2 || L.prep.kmf == 0 || in.minimizer != 1 || in.normals_knn <= L.prep.kmf);
            pid_next += L.n;
        } else if (L.kind == SW_LAUNCH_NORMALS) {
            CHECK(L.n == (int)pl.pids_nrm.size() && L.per >= 1 && L.per <= 32 && L.id_off == 0);
        } else if (L.kind == SW_LAUNCH_SPLIT) {
            CHECK(L.n == pl.n_sync && L.id_off == 0);
        } else {
            while (cls < SW_N_CLASSES && pl.ids[cls].empty())
                ++cls;
            CHECK(cls < SW_N_CLASSES && (cls == SFE_ICP_ROUTE_TINY) == (L.kind == SW_LAUNCH_TINY));
            CHECK(L.id_off == id_next && L.n == (int)pl.ids[cls].size() && L.loop.ox == in.ox);
            for (int k = 0; k < L.n; ++k)
                CHECK(t_ids[id_next + k] == pl.ids[cls][(size_t)k]); // (what the kernel will read there)
            id_next += L.n;
            const SweepLoopBuild &B = L.loop;
            if (L.kind == SW_LAUNCH_LOOP) {
                int b = 0;
                while (b < N_LOOP && !sweep_same_build(B, LOOP_BUILDS[b]))
                    ++b;
                CHECK(b < N_LOOP);
                ++g_loop_hits[b];
                CHECK(B.nt == (cls == SFE_ICP_ROUTE_T0 ? SW_T0_NT : cls == SFE_ICP_ROUTE_T1 ? SW_T1_NT : SW_T2_NT));
                CHECK(B.lds_tgt == (cls <= SFE_ICP_ROUTE_LDS) && B.lds_q == (cls <= SFE_ICP_ROUTE_Q) && B.multi == (cls == SFE_ICP_ROUTE_SPLIT));
                CHECK(B.nt != SW_T2_NT || B.minw == ((pl.wide || B.multi) ? 4 : 8));
                CHECK((!B.rec || rec_chain) && (!B.prof || in.prof));
                // (the Q fit is measured without the profile's counters: a profile build may exceed the share by them)
                const size_t share = B.nt == SW_T2_NT ? pl.lds_share : 160 * 1024;
                CHECK(sweep_plan_ctl_bytes(false, B.rec) + L.body <= share && sweep_plan_ctl_bytes(B.prof, B.rec) + L.body <= 160 * 1024);
                CHECK(L.body == (B.lds_q ? 8 * (size_t)L.t_cap + 6 * (size_t)L.q_cap : 8 * (size_t)L.t_cap) && L.body % 8 == 0);
                CHECK(L.q_cap % 4 == 0 && (B.lds_q || L.q_cap == 0));
            }
            for (int r : pl.ids[cls]) {
                const SweepJob &J = pl.jobs[(size_t)r];
                if (L.kind == SW_LAUNCH_TINY)
                    CHECK(J.n_tgt <= L.t_cap && J.n_src <= L.q_cap && L.t_cap <= SW_TINY_MAX && L.q_cap <= SW_TINY_MAX);
                else if (B.lds_tgt)
                    CHECK(J.n_tgt + SW_PAD <= L.t_cap && (!B.lds_q || J.n_src <= L.q_cap));
                else
                    CHECK(J.n_tgt > SW_TCAP);
            }
            ++cls;
        }
    }
    while (cls < SW_N_CLASSES && pl.ids[cls].empty())
        ++cls;
    CHECK(cls == SW_N_CLASSES && id_next == n_rec);
    int n_listed = 0;
    for (int t = 0; t < 3; ++t)
        n_listed += (int)pl.pids[t].size();
    CHECK(pid_next == n_listed);
    return pl;
}

// {n_src, n_tgt}: the tiers' edges, the Q fit in both LDS shares, the split's edges
static const int SHAPES[][2] = {{64, 64},      {300, 400},   {320, 2048},    {384, 512},     {1000, 2049},   {3000, 3000},
                                {1405, 8192},  {15059, 8192}, {20000, 2100}, {8192, 8193},   {20000, 20000}, // (the pairs: these 11)
                                {1, 1},        {301, 400},   {385, 512},     {384, 513},     {321, 2048},    {2048, 2048},
                                {2049, 2048},  {1406, 8192}, {15058, 8192},  {1000, 8193},   {8191, 8193}};
constexpr int N_SHAPES = sizeof SHAPES / sizeof *SHAPES, N_MIX = 11;

static void add_group(std::vector<int32_t> &jobs4, const int (&s)[2], int count, bool own_targets, int &so, int &to)
{
    for (int k = 0; k < count; ++k) {
        jobs4.insert(jobs4.end(), {so, s[0], to, s[1]});
        if (own_targets && k + 1 < count)
            to += s[1];
    }
    so += s[0], to += s[1];
}

static void sweep_settings(std::vector<int32_t> &jobs4, int n_cu, bool all_flags)
{
    static const int CHAINS[][4] = {{0, 20, 1, 10}, {0, 30, 0, 10}, {0, 11, 0, 10}, {1, 20, 1, 8},
                                    {1, 30, 0, 10}, {1, 20, 1, 12}, {1, 30, 0, 16}}; // minimizer, max_iter, diff checker, knn
    for (const auto &ch : CHAINS)
        for (int tune = 0; tune < 6; ++tune)
            for (int flags = 0; flags < 6; ++flags) {
                if (!all_flags && flags >= 2 && flags <= 4)
                    continue;
                SweepPlanIn in = defaults();
                in.jobs4 = jobs4.data(), in.n_jobs = (int)(jobs4.size() / 4), in.n_cu = n_cu;
                in.minimizer = ch[0], in.max_iter = ch[1], in.use_diff_checker = ch[2], in.normals_knn = ch[3];
                if (tune == 1)
                    in.sw_tiers = in.sw_tiny = 0;
                else if (tune == 2)
                    in.sw_tiny = 0;
                else if (tune == 3)
                    in.sw_multi = 0;
                else if (tune == 4)
                    in.sw_multi_g = 4, in.sw_multi_min_src = 1000, in.sw_multi_share_min = 100;
                else if (tune == 5)
                    in.sw_rec = 0;
                in.prof = flags == 1 || flags == 5, in.ox = flags == 2 || flags == 5, in.no_split = flags == 3;
                in.unsplit = flags == 4, in.side = flags == 5;
                checked_plan(in);
            }
}

static void invariants()
{
    g_what = "grid";
    std::vector<int32_t> jobs4;
    for (int n_cu : {1, 4, 256, 304}) {
        const int counts[] = {1, n_cu, n_cu + 1, 2 * n_cu - 1, 2 * n_cu, 2 * n_cu + 3};
        for (int a = 0; a < N_SHAPES; ++a)
            for (int c : counts) {
                int so = 0, to = 0;
                jobs4.clear();
                add_group(jobs4, SHAPES[a], c, (a + c) % 2 == 1, so, to);
                sweep_settings(jobs4, n_cu, true);
            }
        if (n_cu == 1 || n_cu == 304)
            continue;
        for (int a = 0; a < N_MIX; ++a)
            for (int b = 0; b < N_MIX; ++b)
                for (int cc = 0; cc < 4; ++cc) {
                    int so = 0, to = 0;
                    jobs4.clear();
                    add_group(jobs4, SHAPES[a], (cc & 1) ? 2 * n_cu : 1, a % 2 == 1, so, to);
                    add_group(jobs4, SHAPES[b], (cc & 2) ? 2 * n_cu : 1, b % 2 == 0, so, to);
                    sweep_settings(jobs4, n_cu, false);
                }
    }
}

static const char *const TF[] = {"false", "true"};

// a line: name n_cu minimizer max_iter use_diff_checker normals_knn sw_tiers sw_tiny sw_multi sw_multi_g sw_multi_min_src
// sw_multi_share_min sw_strip_pts sw_rec variant prof ox | groups (n_src n_tgt count)* | runs (route count)* | launches
// (kernel targs workgroups wg_size lds)*
static int fixture(const char *path)
{
    std::ifstream f(path);
    std::string line, name;
    int n = 0;
    while (std::getline(f, line)) {
        g_what = "fixture";
        std::istringstream in_s(line);
        SweepPlanIn in;
        int variant, prof, ox, n_groups, n_runs, n_launches;
        in_s >> name >> in.n_cu >> in.minimizer >> in.max_iter >> in.use_diff_checker >> in.normals_knn >> in.sw_tiers >> in.sw_tiny >>
            in.sw_multi >> in.sw_multi_g >> in.sw_multi_min_src >> in.sw_multi_share_min >> in.sw_strip_pts >> in.sw_rec >> variant >>
            prof >> ox >> n_groups;
        in.sw_cache = 1, in.side = (variant & 8) != 0, in.no_split = (variant & 16) != 0, in.prof = prof != 0, in.ox = ox != 0;
        g_in = in;
        CHECK(!in_s.fail() && n_groups >= 1);
        std::vector<int32_t> jobs4;
        std::vector<std::vector<int32_t>> alone;
        int so = 0, to = 0;
        for (int g = 0; g < n_groups; ++g) {
            int s[2], count;
            in_s >> s[0] >> s[1] >> count;
            CHECK(!in_s.fail());
            add_group(jobs4, s, count, false, so, to);
            alone.push_back({0, s[0], 0, s[1]});
        }
        in.jobs4 = jobs4.data(), in.n_jobs = (int)(jobs4.size() / 4);
        g_what = name.c_str();
        const SweepPlan &pl = checked_plan(in);
        in_s >> n_runs;
        int j = 0;
        for (int r = 0; r < n_runs; ++r) {
            int route, count;
            in_s >> route >> count;
            CHECK(!in_s.fail() && j + count <= in.n_jobs);
            for (int k = 0; k < count; ++k, ++j)
                CHECK(pl.route[(size_t)j] == route);
        }
        CHECK(j == in.n_jobs);
        in_s >> n_launches;
        CHECK(!in_s.fail() && n_launches == pl.n_launches);
        for (int i = 0; i < n_launches; ++i) {
            std::string kernel, targs;
            long long workgroups;
            int wg_size, lds;
            in_s >> kernel >> targs >> workgroups >> wg_size >> lds;
            CHECK(!in_s.fail());
            const SweepLaunch &L = pl.launches[i];
            char want[96];
            const char *want_kernel = "";
            int want_wg = SW_T2_NT, want_lds = 0; // (the static LDS of the kernels, as the trace reports it)
            if (L.kind == SW_LAUNCH_PREP) {
                want_kernel = "icp_sweep_prep_kernel", want_wg = L.prep.nt, want_lds = 512;
                std::snprintf(want, sizeof want, "%d,%d,%d,%s,%d", L.prep.nt, L.prep.tcap, L.prep.gm, TF[L.prep.gtail], L.prep.kmf);
            } else if (L.kind == SW_LAUNCH_NORMALS) {
                want_kernel = "icp_sweep_normals_kernel", want_lds = 1024;
                std::snprintf(want, sizeof want, "%d", SW_T2_NT);
            } else if (L.kind == SW_LAUNCH_SPLIT) {
                want_kernel = "icp_split_kernel", want_lds = 2048;
                std::snprintf(want, sizeof want, "%d", SW_T2_NT);
            } else if (L.kind == SW_LAUNCH_TINY) {
                want_kernel = "icp_tiny_kernel", want_wg = 64;
                std::snprintf(want, sizeof want, "%s", TF[L.loop.ox]);
            } else {
                const SweepLoopBuild &B = L.loop;
                want_kernel = "icp_sweep_kernel", want_wg = B.nt;
                std::snprintf(want, sizeof want, "%d,%d,%s,%s,%s,%s,%s,%s", B.nt, B.minw, TF[B.lds_tgt], TF[B.lds_q], TF[B.prof],
                              TF[B.rec], TF[B.multi], TF[B.ox]);
            }
            CHECK(kernel == want_kernel);
            CHECK(targs == want);
            CHECK(workgroups == (long long)L.n * L.per && wg_size == want_wg && lds == want_lds);
        }
        // the sizes on the two sides of the Q fit come from the header's constants
        const bool fits = name.find("_fits") != std::string::npos;
        if (name.rfind("q_", 0) == 0) {
            const size_t share = (name.find("wide") != std::string::npos ? 160 : 80) * (size_t)1024;
            const int T = jobs4[3], s_max = (int)((share - SW_CTL_Q - 8 * (size_t)(T + SW_PAD) - 16) / 6);
            CHECK(pl.lds_share == share && jobs4[1] == (fits ? s_max : s_max + 1));
            CHECK(pl.route[0] == (fits ? SFE_ICP_ROUTE_Q : SFE_ICP_ROUTE_LDS));
        }
        if (name == "odd_mix") { // each fits alone, together they do not
            CHECK(n_groups == 2 && pl.route[0] == SFE_ICP_ROUTE_LDS && pl.route[1] == SFE_ICP_ROUTE_LDS);
            for (const auto &one : alone) {
                SweepPlanIn in1 = in;
                in1.jobs4 = one.data(), in1.n_jobs = 1;
                g_what = "odd_mix, one job alone";
                CHECK(checked_plan(in1).route[0] == SFE_ICP_ROUTE_Q);
            }
        }
        ++n;
    }
    g_what = "fixture";
    CHECK(n > 0);
    return n;
}

int main(int argc, char **argv)
{
    invariants();
    int unreached = 0;
    for (int b = 0; b < N_LOOP; ++b)
        if (!g_loop_hits[b]) {
            const SweepLoopBuild &B = LOOP_BUILDS[b];
            std::printf("icp_plan_check: no plan of the grid reaches the loop build <%d, %d, %s, %s, %s, %s, %s>: compile time "
                        "spent for nothing?\n", B.nt, B.minw, TF[B.lds_tgt], TF[B.lds_q], TF[B.prof], TF[B.rec], TF[B.multi]);
            ++unreached;
        }
    for (int b = 0; b < N_PREP; ++b)
        if (!g_prep_hits[b]) {
            const SweepPrepBuild &B = PREP_BUILDS[b];
            std::printf("icp_plan_check: no plan of the grid reaches the prep build <%d, %d, %d, %s, %d>: compile time spent for "
                        "nothing?\n", B.nt, B.tcap, B.gm, TF[B.gtail], B.kmf);
            ++unreached;
        }
    g_what = "every listed build is reached", g_in = SweepPlanIn();
    CHECK(unreached == 0);
    const long long grid_plans = g_plans;
    const int n = argc > 1 ? fixture(argv[1]) : 0;
    std::printf("icp_plan_check: ok (%lld plans of the grid; records by class: %lld tiny, %lld one-wave, %lld four-wave, %lld q, %lld lds, "
                "%lld hbm, %lld split shares; %d of %d builds unreached; %d calls of the fixture)\n",
                grid_plans, g_class[0], g_class[1], g_class[2], g_class[3], g_class[4], g_class[5], g_class[6], unreached,
                N_LOOP + N_PREP, n);
    return 0;
}
