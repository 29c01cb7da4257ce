// Strip-sweep ICP, host side: the plan of one call -- the class of every job, the sizes that follow from the classes, the
// build of the loop / prep kernel every launch takes, the layout of the table block and the order of the launches --
// decided once, before the first launch, from a description of the call that holds no device pointer.  Plain C++ without
// a HIP call, so the rules can be run on their own (tests/host/icp_plan_check.cpp).  sfe_icp_sweep.hip executes a plan:
// scratch, waits, the staging copy and the launches.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <map>
#include <utility>
#include <vector>

#include "../../include/sonarfe.h"

#define SW_TCAP 8192   // target points resident in LDS
#define SW_NS_MAX 64   // strips per target
#define SW_PAD (SW_NS_MAX + 4) // sentinels: one in front, one behind every strip, two spare behind the last
#define SW_GRID_MAX 8192 // most cells a target's witness grid can have (built in the prep kernel's LDS: 4 B per cell)
// Job tiers (the scan matches bruce_slam itself produces are 10^2..10^3 points, slam.py:769,1032): the
// same kernels instantiated for one-wave and four-wave workgroups, several jobs per CU, chosen by the plan from
// n_src / n_tgt.  {threads, target capacity of the prep kernel's LDS, witness-grid cells}
#define SW_T0_NT 64
#define SW_T0_TCAP 512
#define SW_T0_GRID 512
#define SW_T1_NT 256
#define SW_T1_TCAP 2048
#define SW_T1_GRID 2048
#define SW_T2_NT 1024 // (= ICP_THREADS; sfe_icp_sweep.hip pins it)
// ... and the most source points of a job of the one-wave / four-wave tier, and of a four-wave job in a call with only
// a few small jobs (one slice of queries and a little: see few_small below)
#define SW_T0_SRC 384
#define SW_T1_SRC 2048
#define SW_T1_FEW_SRC 320
// Many-to-one batches on large clouds (BASELINE configs[4]: 30 guesses x one 20 000 x 20 000 pair, slam.py:346-358): a
// job is split over up to SW_MG_MAX workgroups (queries by strip band), which meet in a per-job sync area
#define SW_MG_MAX 16
#define SW_MG_WORDS 272 // 32-bit words one exchange can carry (a 256-bin histogram + scalars)
// limits of the one-wave kernel the plan sorts jobs by (sfe_icp_tiny.h)
#define SW_TINY_MAX 512        // most points of either cloud
#define SW_TINY_PAIRS_SHORT 400000
#define SW_TINY_PAIRS_LONG 120000
// chains of at least this many iterations, without a differential checker, take the builds with clearance records
// (sfe_icp_sweep.h has what the records are)
#define SW_REC_MIN_ITER 12
#define SW_KNN_MAX 16 // (= ICP_KMAX; sfe_icp_sweep.hip pins it)

struct SweepPrep {
    int tgt_start, n_tgt, ns, pad_;
    long long off;     // offset (points) of this target's slice of the sorted-cloud scratch (stride n_tgt + SW_PAD)
    long long key_off; // targets beyond the LDS capacity: offset of their sort keys in HBM scratch
    long long grid_off; // offset (ints, a multiple of 64) of its witness grid
};

struct SweepJob {
    int src_start, n_src, n_tgt, prep;
    long long tgt_off; // = SweepPrep.off of its target
    long long q_off;   // offset (points) of this job's slice of the per-query scratch
    int out;           // index of the caller's job (guess, T_out, status, iterations) this record works for
    int grp, ngrp;     // split jobs: this record is share `grp` of `ngrp` (1: the whole job)
    int sync;          // ... and their sync area is number `sync`
};

// The builds of the loop kernel: {threads, min waves per EU (the VGPR budget), target in LDS, results in LDS, counted
// profile, clearance records, job shared by several workgroups}; every one exists with and without the outlier modules
// (OX, chosen where it is launched).  sfe_icp_sweep_loop.hip instantiates this list, sfe_icp_sweep.hip finds a plan's
// build key in it, and a key that is not here is an error.  (SW_INSPECT, tools/icp_isa.sh: the bench's build alone, for a
// look at its ISA.)
#ifdef SW_INSPECT
#define SW_LOOP_BUILDS(X) X(SW_T2_NT, 8, true, true, false, true, false)
#else
#define SW_LOOP_BUILDS(X)                                                                                              \
    X(SW_T0_NT, 4, true, true, false, true, false)                                                                     \
    X(SW_T0_NT, 4, true, true, false, false, false)                                                                    \
    X(SW_T1_NT, 4, true, true, true, false, false)                                                                     \
    X(SW_T1_NT, 4, true, true, false, true, false)                                                                     \
    X(SW_T1_NT, 4, true, true, false, false, false)                                                                    \
    X(SW_T2_NT, 4, true, true, false, false, false)                                                                    \
    X(SW_T2_NT, 8, true, true, true, true, false)                                                                      \
    X(SW_T2_NT, 8, true, true, true, false, false)                                                                     \
    X(SW_T2_NT, 8, true, true, false, true, false)                                                                     \
    X(SW_T2_NT, 8, true, true, false, false, false)                                                                    \
    X(SW_T2_NT, 4, true, false, false, false, false)                                                                   \
    X(SW_T2_NT, 8, true, false, true, false, false)                                                                    \
    X(SW_T2_NT, 8, true, false, false, true, false)                                                                    \
    X(SW_T2_NT, 8, true, false, false, false, false)                                                                   \
    X(SW_T2_NT, 4, false, false, false, false, false)                                                                  \
    X(SW_T2_NT, 8, false, false, false, false, false)                                                                  \
    X(SW_T2_NT, 4, false, false, false, false, true)
#endif
// ... and of the prep kernel: {threads, target capacity, witness-grid cells, grid inside the key buffer, capacity of the
// k-NN list (0: chosen at run time)}: the three tiers; the 1024-thread kernel with its witness grid in LDS of its own, or
// inside the key buffer at neighbour-list capacities 8 / 10 (sfe_icp_sweep_prep.hip)
#define SW_PREP_BUILDS(X)                                                                                              \
    X(SW_T0_NT, SW_T0_TCAP, SW_T0_GRID, false, 0)                                                                      \
    X(SW_T1_NT, SW_T1_TCAP, SW_T1_GRID, false, 0)                                                                      \
    X(SW_T2_NT, SW_TCAP, SW_GRID_MAX, false, 0)                                                                        \
    X(SW_T2_NT, SW_TCAP, SW_GRID_MAX, true, 8)                                                                         \
    X(SW_T2_NT, SW_TCAP, SW_GRID_MAX, true, 10)

struct SweepLoopBuild {
    int nt, minw;
    bool lds_tgt, lds_q, prof, rec, multi;
    bool ox; // not in SW_LOOP_BUILDS: both forms of every listed build exist
};
struct SweepPrepBuild {
    int nt, tcap, gm;
    bool gtail;
    int kmf;
};
static inline bool sweep_same_build(const SweepLoopBuild &a, const SweepLoopBuild &b)
{
    return a.nt == b.nt && a.minw == b.minw && a.lds_tgt == b.lds_tgt && a.lds_q == b.lds_q && a.prof == b.prof && a.rec == b.rec &&
           a.multi == b.multi;
}
static inline bool sweep_same_build(const SweepPrepBuild &a, const SweepPrepBuild &b)
{
    return a.nt == b.nt && a.tcap == b.tcap && a.gm == b.gm && a.gtail == b.gtail && a.kmf == b.kmf;
}

// Bytes of the loop kernel's control block (SweepShared, sfe_icp_sweep.h) by build, rounded up to 16: the profile
// counters and the clearance records' transform history only take room in the builds that use them.  The thread count
// does not enter.  sfe_icp_sweep.hip pins every listed build's figure to the struct.
constexpr size_t sweep_plan_ctl_bytes(bool prof, bool rec)
{
    // (15 + 63 more counters of 8 bytes; 63 more rows of 6 + 1 + 1 floats)
    return 5376 + (prof ? (15 + 63) * sizeof(long long) : 0) + (rec ? 63 * 8 * sizeof(float) : 0);
}
// What a job's fit into the Q class is measured with: the largest control block of the LDS_Q builds without the
// profile.  (With the profile on a launch that just fits takes 624 bytes more than its share of 80 KiB, so that a CU
// holds one such workgroup where the plan counts on two: an oversight that only the profile's own timing sees.)
constexpr size_t SW_CTL_Q = sweep_plan_ctl_bytes(false, true);

// What the plan is a pure function of.
struct SweepPlanIn {
    const int32_t *jobs4 = nullptr; // n_jobs x (src_start, n_src, tgt_start, n_tgt) in points (host memory)
    int n_jobs = 0;
    int minimizer = 0, max_iter = 0, use_diff_checker = 0, normals_knn = 0; // of sfe_icp_params
    // of sfe_tuning (sfe_internal.h has what each one is, and the defaults)
    int sw_tiers = 0, sw_tiny = 0, sw_multi = 0, sw_multi_g = 0, sw_multi_min_src = 0, sw_multi_share_min = 1;
    int sw_cache = 0, sw_rec = 0, sw_margin = 0, sw_rtrips = 0, sw_strip_pts = 1, sw_union_iters = 0, sw_union_max = 0;
    int n_cu = 1;
    bool side = false;     // sfe_icp_set_tuning bit 3: tables and preparation on the side stream
    bool no_split = false; // ... bit 4: no job shared by several workgroups
    bool unsplit = false;  // IcpCall::unsplit
    bool prof = false;     // the counted profile is on (sfe_icp_get_profile)
    bool ox = false;       // the chain has MinDist / MedianDist / Bound (sfe_icp_outliers)
};

enum SweepLaunchKind { SW_LAUNCH_PREP, SW_LAUNCH_NORMALS, SW_LAUNCH_SPLIT, SW_LAUNCH_TINY, SW_LAUNCH_LOOP };

struct SweepLaunch {
    SweepLaunchKind kind;
    SweepLoopBuild loop; // SW_LAUNCH_LOOP (SW_LAUNCH_TINY: only .ox)
    SweepPrepBuild prep; // SW_LAUNCH_PREP
    int n;               // workgroups (SW_LAUNCH_NORMALS: n x per)
    int per;             // SW_LAUNCH_NORMALS: workgroups per target
    // its ids start here: in the job ids by class (tiny, loop), the prep ids by tier (prep), pids_nrm (normals), split_first
    int id_off;
    size_t body;         // loop: bytes of LDS behind the control block
    int t_cap, q_cap;    // loop: target / result slots of the LDS layout; tiny: the largest target / source among its jobs
};

#define SW_N_CLASSES 7 // SFE_ICP_ROUTE_TINY .. SFE_ICP_ROUTE_SPLIT: a class's route value is its index
#define SW_MAX_LAUNCHES 13 // three preps, normals, split, tiny, seven loop classes

struct SweepPlan {
    std::vector<SweepPrep> preps;
    std::vector<SweepJob> jobs;
    std::vector<int8_t> route; // SFE_ICP_ROUTE_* of every caller's job
    // Job classes, one launch each:
    //   tiny     clouds of a few hundred points: one wave per job, exhaustive search (sfe_icp_tiny.h)
    //   t0 / t1  small jobs: one-wave / four-wave workgroups, target AND per-query results in LDS, many jobs per CU
    //   q        1024-thread workgroups, target AND per-query results in LDS
    //   lds      ... target in LDS, results in HBM scratch
    //   glb      ... target in HBM scratch (beyond SW_TCAP points)
    //   split    ... target in HBM scratch, the job shared by several workgroups (many-to-one batches on large clouds)
    std::vector<int> ids[SW_N_CLASSES]; // job records by class
    std::vector<int> split_first;       // share-0 record of every split job
    std::vector<int> pids[3];           // targets by prep tier
    std::vector<int> prep_tier;         // ... of every target
    std::vector<char> prep_need; // a target only tiny point-to-point jobs use is not prepared (they take its mean themselves)
    std::vector<int> pids_nrm;   // ... and those whose normals take a kernel of their own
    std::map<std::pair<int, int>, int> seen; // many guesses on one pair share one prep
    long long toff = 0, qoff = 0, koff = 0, goff = 0; // sorted-cloud points, queries, sort keys, witness-grid ints in all
    int n_sync = 0;                                   // sync areas (= split jobs)
    bool wide = false;     // at most one 1024-thread job per CU: those take the whole CU's LDS and 128 VGPRs
    size_t lds_share = 0;  // LDS a 1024-thread workgroup may count on
    int mg = 1;            // most shares of a big job
    bool rec_build = false;
    int sw_cache = 0, sw_cache2 = 0; // the kernel's tuning words
    // the tables travel as ONE block: [preps | job records | job ids by class | share-0 records of the split jobs |
    // prep ids by tier | pids_nrm]
    size_t o_jobs = 0, o_ids = 0, o_split = 0, o_pids = 0, o_pnrm = 0, tab_bytes = 0;
    // prep (by tier), normals, split -- on the preparation's stream -- then tiny and the loop classes on the main stream
    SweepLaunch launches[SW_MAX_LAUNCHES];
    int n_launches = 0, n_prep_launches = 0; // ... the first n_prep_launches of them are the preparation

    // the table block into `h` (tab_bytes of staging)
    void write_tables(char *h) const
    {
        if (!preps.empty())
            memcpy(h, preps.data(), sizeof(SweepPrep) * preps.size());
        if (!jobs.empty())
            memcpy(h + o_jobs, jobs.data(), sizeof(SweepJob) * jobs.size());
        int *hi = (int *)(h + o_ids);
        for (const std::vector<int> &v : ids) {
            if (!v.empty())
                memcpy(hi, v.data(), sizeof(int) * v.size());
            hi += v.size();
        }
        if (!split_first.empty())
            memcpy(h + o_split, split_first.data(), sizeof(int) * split_first.size());
        int *hp = (int *)(h + o_pids);
        for (const std::vector<int> &v : pids) {
            if (!v.empty())
                memcpy(hp, v.data(), sizeof(int) * v.size());
            hp += v.size();
        }
        if (!pids_nrm.empty())
            memcpy(h + o_pnrm, pids_nrm.data(), sizeof(int) * pids_nrm.size());
    }
};

// The kernel's tuning word sw_cache.  (Bits 1..3, 5..7, 25 and 26 are always on: switches of former A/B runs that the
// kernel still tests.)
static inline int sweep_plan_cache_word(const SweepPlanIn &in)
{
    return in.sw_cache |           // bit 0: witness / clearance cache
           2 |                     // bit 1: the cap of a repeated round comes from the queries' upper bounds (else grows 4x)
           4 |                     // bit 2: grid witnesses in the first iteration
           8 |                     // bit 3: witnessed queries skip round 0
           (in.sw_rec ? 16 : 0) |  // bit 4: clearance records
           32 |                    // bit 5: ... with triage passes
           64 |                    // bit 6: first iteration: queries without a witness wait for round 1
           128 |                   // bit 7: later passes: unbounded queries -> cooperative tier
           (in.sw_rtrips << 8) |   // bits 8..15: walk trips per second-pass round
           (in.sw_margin << 16) |  // bits 16..23: margin (percent) of the next iteration's cap over this iteration's limit
           (1 << 25) |             // bit 25: the triage pass as a loop of its own
           (1 << 26);              // bit 26: steady state: the trimmed quantile looked for around the previous one
}

// Fills `pl` (whatever it held is overwritten; its vectors keep their capacity).
static inline void sweep_plan(const SweepPlanIn &in, SweepPlan &pl)
{
    const int n_jobs = in.n_jobs;
    const int32_t *jobs4 = in.jobs4;
    pl.preps.clear();
    pl.jobs.clear();
    pl.jobs.reserve((size_t)n_jobs);
    for (std::vector<int> &v : pl.ids)
        v.clear();
    for (std::vector<int> &v : pl.pids)
        v.clear();
    pl.split_first.clear();
    pl.prep_tier.clear();
    pl.prep_need.clear();
    pl.pids_nrm.clear();
    pl.seen.clear();
    pl.toff = pl.qoff = pl.koff = pl.goff = 0;
    pl.n_sync = 0;
    pl.n_launches = pl.n_prep_launches = 0;
    std::vector<int> &ids_tiny = pl.ids[SFE_ICP_ROUTE_TINY], &ids_t0 = pl.ids[SFE_ICP_ROUTE_T0], &ids_t1 = pl.ids[SFE_ICP_ROUTE_T1],
                     &ids_q = pl.ids[SFE_ICP_ROUTE_Q], &ids_lds = pl.ids[SFE_ICP_ROUTE_LDS], &ids_glb = pl.ids[SFE_ICP_ROUTE_GLB],
                     &ids_multi = pl.ids[SFE_ICP_ROUTE_SPLIT];
    // (tuning sw_tiers = 0 sends every job to the 1024-thread kernels)
    // large jobs shared by several workgroups unless tuning sw_multi = 0, sfe_icp_set_tuning bit 4 or the call is the
    // unsplit second run (a device shared with another context / process cannot promise that all shares of a job are
    // resident together: ADVICE r3)
    const bool multi_on = in.sw_multi && !in.no_split && !in.unsplit;
    // ~96 points per strip on average (tuning sw_strip_pts; measured optimum 96-128 on 5000-point clouds: fewer queries need
    // a second strip, a little more to walk in each), one strip (= a plain x sweep) for small clouds
    const int strip_pts = in.sw_strip_pts;
    // clouds of a few hundred points: the exhaustive one-wave kernel (tuning sw_tiny)
    const long long tiny_pairs = (in.use_diff_checker || in.max_iter < SW_REC_MIN_ITER) ? SW_TINY_PAIRS_SHORT : SW_TINY_PAIRS_LONG;
    auto is_tiny = [&](int n_src, int n_tgt) {
        return in.sw_tiny && n_src <= SW_TINY_MAX && n_tgt <= SW_TINY_MAX && (long long)n_src * n_tgt <= tiny_pairs;
    };

    // The small workgroups buy throughput (many jobs per CU), not latency: ONE scan match of 200 points is done sooner by
    // 256 threads (one slice of queries per pass) than by 64 (four slices, one after the other).  So the one-wave tier is
    // only used when the call brings enough such jobs to fill the device with them (the live node's single scan
    // match takes the four-wave kernel).
    auto fits0 = [&](int n_src, int n_tgt) { return in.sw_tiers && n_src <= SW_T0_SRC && n_tgt <= SW_T0_TCAP; };
    auto fits1 = [&](int n_src, int n_tgt) { return in.sw_tiers && n_src <= SW_T1_SRC && n_tgt <= SW_T1_TCAP; };
    // (Jobs that the tiny kernel takes are counted here too, although they never reach a small tier: 2 n_cu tiny jobs
    // make the one-wave tier live for a single job beside them that is not tiny.  It looks like an oversight; the
    // measurements below were taken with it.)
    int n_fit0 = 0, n_fit1 = 0;
    for (int j = 0; j < n_jobs; ++j) {
        const int32_t *q = jobs4 + 4 * (size_t)j;
        if (fits0(q[1], q[3]))
            ++n_fit0;
        else if (fits1(q[1], q[3]))
            ++n_fit1;
    }
    const bool use_t0 = n_fit0 >= 2 * in.n_cu;
    const bool use_t1 = n_fit1 + (use_t0 ? 0 : n_fit0) >= 1;
    // ... and with only a few small jobs in the call the four-wave kernel takes those of at most one slice of queries
    // (measured, one scan match alone: 200 points 261 us with 256 threads, 282 with 1024, 464 with 64; 1000 points 508 us
    // with 256 threads, 341 with 1024)
    const bool few_small = n_fit0 + n_fit1 < 2 * in.n_cu;
    // first pass: sizes -> how many big jobs there are (decides `wide` and whether big jobs are split)
    int n_big = 0, n_t2 = 0;
    auto tier_of = [&](int n_src, int n_tgt) {
        if (use_t0 && fits0(n_src, n_tgt))
            return 0;
        if (use_t1 && fits1(n_src, n_tgt) && (!few_small || n_src <= SW_T1_FEW_SRC))
            return 1;
        return 2;
    };
    for (int j = 0; j < n_jobs; ++j) {
        const int32_t *q = jobs4 + 4 * (size_t)j;
        if (!is_tiny(q[1], q[3]) && tier_of(q[1], q[3]) == 2) {
            ++n_t2;
            if (q[3] > SW_TCAP && q[1] >= in.sw_multi_min_src)
                ++n_big;
        }
    }
    // LDS share of a 1024-thread workgroup: two per CU when the batch has more jobs than CUs, else the whole CU
    pl.wide = n_t2 <= in.n_cu;
    const bool wide = pl.wide;
    const size_t lds_share = pl.lds_share = (wide ? 160 : 80) * (size_t)1024;
    // Shares per big job: all workgroups of the launch must be resident at once (one 128-VGPR workgroup per CU) -- only
    // when the 1024-thread jobs of this call are the big ones alone and G x n_big fits the CUs
    int mg = 1;
    if (multi_on && n_big > 0 && n_big == n_t2 && wide) {
        mg = std::min(SW_MG_MAX, in.n_cu / n_big);
        if (in.sw_multi_g > 0) // (tuning: shares per job)
            mg = std::min(in.sw_multi_g, std::max(1, in.n_cu / n_big));
    }
    pl.mg = mg;
    constexpr size_t ctl_q = SW_CTL_Q;
    int q_tmax = 0, q_smax = 0, t0_tmax = 0, t0_smax = 0, t1_tmax = 0, t1_smax = 0, tiny_tmax = 0, tiny_smax = 0;
    pl.route.resize((size_t)n_jobs); // the class of every job, for sfe_icp_last_routes
    int8_t *route = pl.route.data();
    for (int j = 0; j < n_jobs; ++j) {
        const int32_t *q = jobs4 + 4 * (size_t)j;
        const auto key = std::make_pair((int)q[2], (int)q[3]);
        auto it = pl.seen.find(key);
        if (it == pl.seen.end()) {
            it = pl.seen.emplace(key, (int)pl.preps.size()).first;
            long long n2 = 0;
            if (q[3] > SW_TCAP) {
                n2 = 2;
                while (n2 < q[3])
                    n2 <<= 1;
            }
            const int n_strips = std::max(1, std::min(SW_NS_MAX, (int)q[3] / strip_pts));
            // (the target's preparation follows the same rule: one wave only when the call fills the device with such jobs.
            // Only its own size enters, not the tier of the jobs that use it: with few_small a 300-point target of a
            // 1000-point source is prepared by the four-wave kernel for a 1024-thread job, and the target of a tiny
            // point-to-plane job by whichever tier is live.)
            const int pt = (use_t0 && q[3] <= SW_T0_TCAP) ? 0 : ((use_t1 && q[3] <= SW_T1_TCAP) ? 1 : 2);
            pl.prep_tier.push_back(pt);
            pl.prep_need.push_back(0);
            // (targets sorted in HBM scratch get their normals from icp_sweep_normals_kernel: pad_ = 1)
            const int nrm_later = (q[3] > SW_TCAP && in.minimizer == 1) ? 1 : 0;
            if (nrm_later)
                pl.pids_nrm.push_back((int)pl.preps.size());
            pl.preps.push_back({q[2], q[3], n_strips, nrm_later, pl.toff, pl.koff, pl.goff});
            pl.toff += q[3] + SW_PAD;
            pl.koff += n2;
            pl.goff += pt == 0 ? SW_T0_GRID : (pt == 1 ? SW_T1_GRID : SW_GRID_MAX);
        }
        const SweepPrep &pr = pl.preps[(size_t)it->second];
        const bool tiny = is_tiny(q[1], q[3]);
        const int tier = tiny ? -1 : tier_of(q[1], q[3]);
        if (!tiny || in.minimizer == 1)
            pl.prep_need[(size_t)it->second] = 1;
        int shares = 1;
        if (tier == 2 && mg > 1 && q[3] > SW_TCAP && q[1] >= in.sw_multi_min_src)
            shares = std::max(1, std::min(mg, (int)q[1] / in.sw_multi_share_min));
        const int rec0 = (int)pl.jobs.size();
        for (int g = 0; g < shares; ++g) // (the shares of a split job: the split kernel fills in their clouds)
            pl.jobs.push_back({q[0], q[1], q[3], it->second, pr.off, pl.qoff, j, g, shares, shares > 1 ? pl.n_sync : 0});
        pl.qoff += q[1];
        if (shares > 1) {
            pl.split_first.push_back(rec0);
            for (int g = 0; g < shares; ++g)
                ids_multi.push_back(rec0 + g);
            ++pl.n_sync;
            route[j] = SFE_ICP_ROUTE_SPLIT;
        } else if (tiny) {
            ids_tiny.push_back(rec0);
            route[j] = SFE_ICP_ROUTE_TINY;
            tiny_tmax = std::max(tiny_tmax, (int)q[3]);
            tiny_smax = std::max(tiny_smax, (int)q[1]);
        } else if (tier == 0) {
            ids_t0.push_back(rec0);
            route[j] = SFE_ICP_ROUTE_T0;
            t0_tmax = std::max(t0_tmax, (int)q[3]);
            t0_smax = std::max(t0_smax, (int)q[1]);
        } else if (tier == 1) {
            ids_t1.push_back(rec0);
            route[j] = SFE_ICP_ROUTE_T1;
            t1_tmax = std::max(t1_tmax, (int)q[3]);
            t1_smax = std::max(t1_smax, (int)q[1]);
        } else {
            const bool fits_q = q[3] <= SW_TCAP &&
                                ctl_q + 8 * (size_t)(q[3] + SW_PAD) + 6 * (size_t)q[1] + 16 <= lds_share;
            if (fits_q) {
                ids_q.push_back(rec0);
                route[j] = SFE_ICP_ROUTE_Q;
                q_tmax = std::max(q_tmax, (int)q[3]);
                q_smax = std::max(q_smax, (int)q[1]);
            } else {
                (q[3] <= SW_TCAP ? ids_lds : ids_glb).push_back(rec0);
                route[j] = q[3] <= SW_TCAP ? SFE_ICP_ROUTE_LDS : SFE_ICP_ROUTE_GLB;
            }
        }
    }
    for (size_t pid = 0; pid < pl.preps.size(); ++pid)
        if (pl.prep_need[pid])
            pl.pids[pl.prep_tier[pid]].push_back((int)pid);
    // the LDS_Q launch is sized by the largest target and the largest source among its jobs
    const int t_cap = q_tmax + SW_PAD, q_cap = (q_smax + 3) & ~3;
    if (!ids_q.empty() && ctl_q + 8 * (size_t)t_cap + 6 * (size_t)q_cap > lds_share) {
        ids_lds.insert(ids_lds.end(), ids_q.begin(), ids_q.end()); // odd mix of shapes: keep the results in HBM
        for (int r : ids_q)
            route[pl.jobs[(size_t)r].out] = SFE_ICP_ROUTE_LDS;
        std::sort(ids_lds.begin(), ids_lds.end());
        ids_q.clear();
    }
    const size_t n_prep = pl.preps.size(), n_rec = pl.jobs.size();
    pl.o_jobs = (sizeof(SweepPrep) * n_prep + 15) & ~(size_t)15;
    pl.o_ids = (pl.o_jobs + sizeof(SweepJob) * n_rec + 15) & ~(size_t)15;
    pl.o_split = pl.o_ids + sizeof(int) * n_rec;
    pl.o_pids = pl.o_split + sizeof(int) * pl.split_first.size();
    pl.o_pnrm = pl.o_pids + sizeof(int) * n_prep;
    pl.tab_bytes = pl.o_pnrm + sizeof(int) * pl.pids_nrm.size();

    pl.sw_cache = sweep_plan_cache_word(in);
    // union scan of the first iterations: bits 0..7 = iterations that use it, bits 8..23 = most points of a union window.
    // Measured (1024 jobs of 5000 x 5000, search cycles of workgroup 0 per iteration, walks -> union): iteration 0
    // 997 k -> 828 k, iteration 1 486 k -> 659 k, iteration 2 324 k -> 585 k: only the first iteration's windows (bounds
    // from grid witnesses, ~0.9 m) are wide enough for the union of 64 neighbours' windows (~400 points) to beat the
    // private walks; from the second iteration on a query's old neighbour bounds it to a few dozen candidates.  Whole
    // launch: p2plane30 8.78-8.87 -> 8.64-8.76 ms, shipped chain 4.07 -> 3.93-4.00 ms per 1024 jobs.
    pl.sw_cache2 = in.sw_union_iters | (in.sw_union_max << 8);
    // The build with clearance records carries more per-lane state (the 64-VGPR budget makes every register count:
    // the same chain ran ~10 % slower in it until the records start to hit; since the walks of the iterations before
    // that are an instance of their own without the records' bookkeeping, a 12-iteration chain on the bench's pairs,
    // whose records hit from iteration 9 on, takes 15.55 ms per 4096 jobs in it and 16.30 ms in the build without --
    // it was 16.48 against 16.29, profiles/icp_walk_modes_times.txt), so it only takes chains that are set to
    // run many iterations: a fixed count (no differential checker) of at least SW_REC_MIN_ITER -- and only the builds
    // with LDS-resident targets: for the one-workgroup-per-CU builds with the target in HBM (30 guesses x one
    // 20 000 x 20 000 pair) the records cost more than they save (24.6 -> 30.9 ms, tools/hires_times.py).
    const bool rec = pl.rec_build = (pl.sw_cache & 16) != 0 && in.max_iter >= SW_REC_MIN_ITER && !in.use_diff_checker;
    const bool prof = in.prof, ox = in.ox;

    // ---- the launches ----
    auto add = [&](SweepLaunchKind kind, int n, int id_off) -> SweepLaunch & {
        SweepLaunch &L = pl.launches[pl.n_launches++];
        L = SweepLaunch{};
        L.kind = kind, L.n = n, L.per = 1, L.id_off = id_off;
        return L;
    };
    const int np0 = (int)pl.pids[0].size(), np1 = (int)pl.pids[1].size(), np2 = (int)pl.pids[2].size();
    if (np0)
        add(SW_LAUNCH_PREP, np0, 0).prep = {SW_T0_NT, SW_T0_TCAP, SW_T0_GRID, false, 0};
    if (np1)
        add(SW_LAUNCH_PREP, np1, np0).prep = {SW_T1_NT, SW_T1_TCAP, SW_T1_GRID, false, 0};
    if (np2) {
        // (the list capacity the kernel is built for: the smallest of 8 / 10 / 12 / 16 that holds normals_knn)
        const int km = in.minimizer != 1 ? 8 : in.normals_knn <= 8 ? 8 : in.normals_knn <= 10 ? 10 : in.normals_knn <= 12 ? 12 : SW_KNN_MAX;
        // (lists of 12 / 16 neighbours do not fit 64 registers: 184 / 541 spills; those keep one workgroup per CU)
        add(SW_LAUNCH_PREP, np2, np0 + np1).prep = km > 10 ? SweepPrepBuild{SW_T2_NT, SW_TCAP, SW_GRID_MAX, false, 0}
                                                           : SweepPrepBuild{SW_T2_NT, SW_TCAP, SW_GRID_MAX, true, km};
    }
    if (!pl.pids_nrm.empty()) { // behind the prep (sorted cloud, strip table), 1024 points per workgroup and pass
        int tmax = 0;
        for (int pid : pl.pids_nrm)
            tmax = std::max(tmax, pl.preps[(size_t)pid].n_tgt);
        const int n = (int)pl.pids_nrm.size();
        add(SW_LAUNCH_NORMALS, n, 0).per =
            std::max(1, std::min(32, std::min((tmax + 2 * SW_T2_NT - 1) / (2 * SW_T2_NT), std::max(1, 2 * in.n_cu / n))));
    }
    if (!pl.split_first.empty()) // behind the prep (it needs the strip tables), in front of the loop
        add(SW_LAUNCH_SPLIT, (int)pl.split_first.size(), 0);
    pl.n_prep_launches = pl.n_launches;

    // A/B: VGPR budget of the LDS_Q build.  A workgroup is 1024 threads = 4 waves per SIMD, so two workgroups per CU
    // only fit at <= 64 VGPRs: measured (4096 jobs of 5000 x 5000, p2plane30) 64 VGPRs 35.4 ms, 72 VGPRs 51.4 ms,
    // 128 VGPRs 48.6 ms (profiles/r02_icp_vgpr_budget.txt) -- one resident job per CU costs more than the 86 spilled
    // VGPRs of the 64-VGPR build
    int off = 0;
    auto loop = [&](const std::vector<int> &v, SweepLoopBuild b, size_t body, int tc, int qc) {
        if (v.empty())
            return;
        SweepLaunch &L = add(SW_LAUNCH_LOOP, (int)v.size(), off);
        b.ox = ox;
        L.loop = b, L.body = body, L.t_cap = tc, L.q_cap = qc;
        off += (int)v.size();
    };
    if (!ids_tiny.empty()) { // one wave per job, everything in LDS (sfe_icp_tiny.h)
        SweepLaunch &L = add(SW_LAUNCH_TINY, (int)ids_tiny.size(), off);
        L.loop.ox = ox, L.t_cap = tiny_tmax, L.q_cap = tiny_smax;
        off += L.n;
    }
    { // one wave per job (no workgroup barrier costs anything), 128 VGPRs, up to 16 jobs per CU.  (The profile has no
      // one-wave build: it is not counted there.)
        const int tc = t0_tmax + SW_PAD, qc = (t0_smax + 3) & ~3;
        loop(ids_t0, {SW_T0_NT, 4, true, true, false, rec, false, false}, 8 * (size_t)tc + 6 * (size_t)qc, tc, qc);
    }
    { // four waves per job, 128 VGPRs, up to 4 jobs per CU.  (There is no build with the profile AND the records: a chain
      // that takes the records is not counted here, while the Q class below has that build.)
        const int tc = t1_tmax + SW_PAD, qc = (t1_smax + 3) & ~3;
        loop(ids_t1, {SW_T1_NT, 4, true, true, prof && !rec, rec, false, false}, 8 * (size_t)tc + 6 * (size_t)qc, tc, qc);
    }
    // 1024-thread jobs: up to one job per CU the 128-VGPR build wins (no spills, measured +8 %), beyond that two
    // 64-VGPR workgroups per CU overlap each other's serial phases (measured +14 % at 512 jobs).  (The 128-VGPR builds
    // exist without records and without the profile only: with `wide` a 30-iteration chain runs without its records and
    // the profile counts nothing.  The records may be an oversight -- the register argument above is about 64 VGPRs.)
    loop(ids_q, wide ? SweepLoopBuild{SW_T2_NT, 4, true, true, false, false, false, false}
                     : SweepLoopBuild{SW_T2_NT, 8, true, true, prof, rec, false, false},
         8 * (size_t)t_cap + 6 * (size_t)q_cap, t_cap, q_cap);
    // (results in HBM, two workgroups per CU: the profile wins over the records -- there is no build with both)
    loop(ids_lds, wide ? SweepLoopBuild{SW_T2_NT, 4, true, false, false, false, false, false}
                       : SweepLoopBuild{SW_T2_NT, 8, true, false, prof, rec && !prof, false, false},
         8 * (size_t)(SW_TCAP + SW_PAD), SW_TCAP + SW_PAD, 0);
    // Targets beyond SW_TCAP points stay in HBM scratch and are read through L2.  (Rounds 3-4 carried a build that held the
    // strips around a workgroup's queries in LDS instead -- 7.97 ms with it, 7.82 without on 30 guesses x one 20 000 x 20 000
    // pair: the target is L2-resident and sixteen waves hide its latency, while every read paid the window test; removed in
    // round 5, profiles/r05_pruned_variants.txt.)  Without a window the LDS behind the control block only serves the query sort.
    loop(ids_glb, {SW_T2_NT, wide ? 4 : 8, false, false, false, false, false, false}, 8 * (size_t)SW_TCAP, SW_TCAP, 0);
    // every share on a CU of its own, all of them resident (mg x n_big <= CUs); their clouds were gathered
    loop(ids_multi, {SW_T2_NT, 4, false, false, false, false, true, false}, 8 * (size_t)SW_TCAP, SW_TCAP, 0);
}
