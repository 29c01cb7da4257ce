// Strip-sweep ICP, host side: executes the plan of a call (sfe_icp_sweep_plan.h: the jobs sorted into classes, the build of
// every launch, the tables' layout, the order of the launches) -- scratch, stream waits, the table copy, the launches
// (preparation -- optionally on the side stream -- normals, split, loop), events.  The kernels live in
// sfe_icp_sweep_prep.hip and sfe_icp_sweep_loop.hip; what they share, the exactness argument of the search and the
// overview are in sfe_icp_sweep.h.
#include "sfe_icp_sweep.h"

#include <vector>

static_assert(SW_T2_NT == ICP_THREADS && SW_KNN_MAX == ICP_KMAX, "sfe_icp_sweep_plan.h restates them");
static_assert(SW_CTL_Q == sweep_ctl_bytes<ICP_THREADS, false, true>(), "the Q class is measured with this control block");
#define SW_X(NT, MINW, LT, LQ, PROF, REC, MULTI) \
    static_assert(sweep_plan_ctl_bytes(PROF, REC) == sweep_ctl_bytes<NT, PROF, REC>(), "sweep_plan_ctl_bytes");
SW_LOOP_BUILDS(SW_X)
#undef SW_X

// a plan's build key -> the instantiation of that build (SW_LOOP_BUILDS / SW_PREP_BUILDS); a key that is not listed is
// an error of the plan
static int sweep_dispatch_loop(const SweepLoopBuild &b, const SweepLaunchArgs &a, int n, const int *d_ids, size_t body, int t_cap,
                               int q_cap)
{
#define SW_X(NT, MINW, LT, LQ, PROF, REC, MULTI)                                                                        \
    if (sweep_same_build(b, SweepLoopBuild{NT, MINW, LT, LQ, PROF, REC, MULTI, false}))                               \
        return sweep_launch_loop<NT, MINW, LT, LQ, PROF, REC, MULTI>(a, n, d_ids, body, t_cap, q_cap);
    SW_LOOP_BUILDS(SW_X)
#undef SW_X
    return sfe_set_err(a.ctx, SFE_ERR_ARG, "sfe_icp_sweep: no loop build <%d, %d, %d, %d, %d, %d, %d> (SW_LOOP_BUILDS)", b.nt, b.minw,
                       (int)b.lds_tgt, (int)b.lds_q, (int)b.prof, (int)b.rec, (int)b.multi);
}

static int sweep_dispatch_prep(const SweepPrepBuild &b, sfe_ctx *ctx, hipStream_t ps, const sfe_icp_params *p, int n,
                               const SweepPrep *d_preps, const int *d_pids, const float2 *d_tgt, float2 *d_stgt, int *d_perm,
                               float2 *d_snrm, float *d_mean, unsigned long long *d_gkeys, StripTab *d_tab, int *d_grid)
{
#define SW_X(NT, TCAP, GM, GTAIL, KMF)                                                                                  \
    if (sweep_same_build(b, SweepPrepBuild{NT, TCAP, GM, GTAIL, KMF}))                                                 \
        return sweep_launch_prep<NT, TCAP, GM, GTAIL, KMF>(ctx, ps, p, n, d_preps, d_pids, d_tgt, d_stgt, d_perm, d_snrm, d_mean, \
                                                           d_gkeys, d_tab, d_grid);
    SW_PREP_BUILDS(SW_X)
#undef SW_X
    return sfe_set_err(ctx, SFE_ERR_ARG, "sfe_icp_sweep: no prep build <%d, %d, %d, %d, %d> (SW_PREP_BUILDS)", b.nt, b.tcap, b.gm,
                       (int)b.gtail, b.kmf);
}

// ---------------------------------------------------------------------------------------------
// host side: the plan of the call (sfe_icp_sweep_plan.h), then scratch, waits, the table copy and the plan's launches.
// jobs4 = n_jobs x (src_start, n_src, tgt_start, n_tgt) in points.
// ---------------------------------------------------------------------------------------------
int sfe_icp_sweep_launch(sfe_ctx *ctx, const sfe_icp_params *p, const IcpCall &call, const float *d_src, const float *d_tgt,
                         const int32_t *jobs4, const float *d_guess9, int n_jobs, float *d_T9, int32_t *d_status,
                         int32_t *d_iters)
{
    const sfe_tuning &tu = ctx->tune;
    SweepPlanIn in;
    in.jobs4 = jobs4, in.n_jobs = n_jobs;
    in.minimizer = p->minimizer, in.max_iter = p->max_iter, in.use_diff_checker = p->use_diff_checker, in.normals_knn = p->normals_knn;
    in.sw_tiers = tu.sw_tiers, in.sw_tiny = tu.sw_tiny, in.sw_multi = tu.sw_multi, in.sw_multi_g = tu.sw_multi_g;
    in.sw_multi_min_src = tu.sw_multi_min_src, in.sw_multi_share_min = tu.sw_multi_share_min;
    in.sw_cache = tu.sw_cache, in.sw_rec = tu.sw_rec, in.sw_margin = tu.sw_margin, in.sw_rtrips = tu.sw_rtrips;
    in.sw_strip_pts = tu.sw_strip_pts, in.sw_union_iters = tu.sw_union_iters, in.sw_union_max = tu.sw_union_max;
    in.n_cu = ctx->n_cu;
    // Tuning bit 3: the caller vouches that the clouds and guesses of this batch are final (nothing enqueued on
    // ctx->stream still writes them).  The job tables and the preparation kernels then go to the side stream and write
    // generation g of their scratch, while the loop kernel of the batch before may still read the other one
    // (sfe_icp_gen.h).  Without the bit: generation 0, everything on ctx->stream.
    in.side = (ctx->icp_variant & 8) != 0;
    in.no_split = (ctx->icp_variant & 16) != 0;
    in.unsplit = call.unsplit;
    in.prof = ctx->icp_prof != 0;
    in.ox = call.ox.use_min_dist || call.ox.use_median || call.ox.use_bound;
    SweepPlan pl;
    pl.route.swap(ctx->icp_routes); // (its buffer serves again)
    sweep_plan(in, pl);
    ctx->icp_routes.swap(pl.route); // the class of every job, for sfe_icp_last_routes
    const bool side = in.side;
    const int n_prep = (int)pl.preps.size(), n_split = (int)pl.split_first.size();
    const long long toff = pl.toff, qoff = pl.qoff;
    const SfeIcpGenPlan gen = sfe_icp_gen_begin(ctx->icp_gens, side, n_split > 0);
    if (gen.sync_first) { // the launch before returned an error half-way: what it left on the streams is in no event
        SFE_HIP(ctx, hipStreamSynchronize(ctx->stream2));
        SFE_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    // scratch slots of what the preparation writes and the loop reads, by generation.  (A slot that grows waits for
    // every stream of the context before it frees its block: sfe_scratch.)
    enum { G_TABLES, G_STGT, G_PERM, G_SNRM, G_MEAN, G_GKEYS, G_TAB, G_GRID, G_N };
    static const int gen_slot[2][G_N] = {{12, 14, 15, 16, 17, 24, 23, 38}, {72, 73, 74, 75, 76, 77, 78, 79}};
    static_assert(SFE_NSCRATCH == 81, "generation 1 takes slots 72..79, the loop kernel's slot records the last one");
    const int *gs = gen_slot[gen.g];
    char *d_tables = (char *)sfe_scratch(ctx, gs[G_TABLES], pl.tab_bytes);
    float2 *d_stgt = (float2 *)sfe_scratch(ctx, gs[G_STGT], sizeof(float2) * (size_t)toff);
    int *d_perm = (int *)sfe_scratch(ctx, gs[G_PERM], sizeof(int) * (size_t)toff);
    float2 *d_snrm = p->minimizer == 1 ? (float2 *)sfe_scratch(ctx, gs[G_SNRM], sizeof(float2) * (size_t)toff) : nullptr;
    float *d_mean = (float *)sfe_scratch(ctx, gs[G_MEAN], sizeof(float) * 2 * (size_t)n_prep);
    unsigned long long *d_gkeys =
        (unsigned long long *)sfe_scratch(ctx, gs[G_GKEYS], sizeof(unsigned long long) * (size_t)std::max(pl.koff, 1LL));
    int4 *d_qst = (int4 *)sfe_scratch(ctx, 19, sizeof(int4) * (size_t)qoff);
    // per query: 5 ints of work lists and the slot index, the guess-frame position under the query's own index and the
    // 16-byte slot record (20 + 8 + 16 B; the order, record and sorted-source arrays these replace were 28 + 8 B)
    int *d_qwl = (int *)sfe_scratch(ctx, 21, sizeof(int) * 5 * (size_t)qoff);
    float2 *d_qrsrc = (float2 *)sfe_scratch(ctx, 30, sizeof(float2) * (size_t)qoff);
    SweepSlot *d_qslot = (SweepSlot *)sfe_scratch(ctx, 80, sizeof(SweepSlot) * (size_t)qoff);
    StripTab *d_tab = (StripTab *)sfe_scratch(ctx, gs[G_TAB], sizeof(StripTab) * (size_t)n_prep);
    int *d_grid = (int *)sfe_scratch(ctx, gs[G_GRID], sizeof(int) * (size_t)pl.goff);
    float *d_nn_d2 = (float *)sfe_scratch(ctx, 5, sizeof(float) * (size_t)qoff);
    int *d_nn_pos = (int *)sfe_scratch(ctx, 6, sizeof(int) * (size_t)qoff);
    if (!d_tables || !d_stgt || !d_perm || (p->minimizer == 1 && !d_snrm) || !d_mean || !d_gkeys || !d_qst || !d_qwl || !d_qrsrc || !d_qslot || !d_tab || !d_grid ||
        !d_nn_d2 || !d_nn_pos)
        return SFE_ERR_HIP;
    // split jobs: the gathered source clouds of the shares and the sync areas (one generation: a preparation that
    // writes them waits for every earlier loop kernel)
    float2 *d_gsrc = nullptr;
    unsigned long long *d_sync = nullptr;
    const size_t sync_bytes = sizeof(unsigned long long) * 2 * SW_MG_MAX * SW_MG_WORDS * (size_t)pl.n_sync;
    if (n_split) {
        d_gsrc = (float2 *)sfe_scratch(ctx, 46, sizeof(float2) * (size_t)qoff);
        d_sync = (unsigned long long *)sfe_scratch(ctx, 45, sync_bytes);
        if (!d_gsrc || !d_sync)
            return SFE_ERR_HIP;
    }
    SweepPrep *d_preps = (SweepPrep *)d_tables;
    SweepJob *d_jobs = (SweepJob *)(d_tables + pl.o_jobs);
    const int *d_ids = (const int *)(d_tables + pl.o_ids);
    const int *d_split = (const int *)(d_tables + pl.o_split);
    const int *d_pids = (const int *)(d_tables + pl.o_pids);
    const int *d_pnrm = (const int *)(d_tables + pl.o_pnrm);
    // The side stream has the lowest priority: the preparation takes the workgroup slots that whatever runs on
    // ctx->stream leaves free -- the loop kernel of the batch before, for its whole length, then the front end that a batch
    // pipeline enqueues there for the same step; the loop kernel of this batch waits for it (ev_prep).
    hipStream_t ps = side ? ctx->stream2 : ctx->stream;
    for (int g = 0; g < 2; ++g) // the loop kernels that still read what this preparation rewrites
        if (gen.wait[g])
            SFE_HIP(ctx, hipStreamWaitEvent(ps, ctx->ev_loop[g], 0));
    if (gen.wait_begin) // ... and it starts with the newest loop kernel, not with what is enqueued in front of that
        SFE_HIP(ctx, hipStreamWaitEvent(ps, ctx->ev_loop_begin, 0));
    { // pinned staging (no stream synchronisation: this entry point only enqueues)
        char *h = (char *)sfe_pinned_begin(ctx, pl.tab_bytes);
        if (!h)
            return SFE_ERR_HIP;
        pl.write_tables(h);
        SFE_HIP(ctx, hipMemcpyAsync(d_tables, h, pl.tab_bytes, hipMemcpyHostToDevice, ps));
        if (int rc = sfe_pinned_end(ctx, ps))
            return rc;
    }
    for (int i = 0; i < pl.n_prep_launches; ++i) { // the preparation: prep by tier, normals, split
        const SweepLaunch &L = pl.launches[i];
        int rc = 0;
        if (L.kind == SW_LAUNCH_PREP) {
            rc = sweep_dispatch_prep(L.prep, ctx, ps, p, L.n, d_preps, d_pids + L.id_off, (const float2 *)d_tgt, d_stgt, d_perm, d_snrm,
                                     d_mean, d_gkeys, d_tab, d_grid);
        } else if (L.kind == SW_LAUNCH_NORMALS) {
            rc = sweep_launch_normals(ctx, ps, p, L.n, L.per, d_preps, d_pnrm, (const float2 *)d_stgt, (const int *)d_perm, d_snrm,
                                      (const StripTab *)d_tab);
        } else {
            SFE_HIP(ctx, hipMemsetAsync(d_sync, 0, sync_bytes, ps));
            rc = sweep_launch_split(ctx, ps, L.n, d_jobs, d_split, (const float2 *)d_src, d_guess9, d_mean, d_tab, d_gsrc);
        }
        if (rc)
            return rc;
    }
    if (side) {
        SFE_HIP(ctx, hipEventRecord(ctx->ev_prep, ps));
        SFE_HIP(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_prep, 0));
    }
    const bool debug = tu.icp_debug != 0;
    int *d_dbg = nullptr;
    if (debug) {
        d_dbg = (int *)sfe_scratch(ctx, 22, sizeof(int) * 8);
        if (!d_dbg)
            return SFE_ERR_HIP;
        SFE_HIP(ctx, hipMemsetAsync(d_dbg, 0, sizeof(int) * 8, ctx->stream));
    }
    long long *d_prof = in.prof ? (long long *)sfe_scratch(ctx, 20, sizeof(long long) * SFE_ICP_PROF_N) : nullptr;
    if (in.prof && !d_prof)
        return SFE_ERR_HIP;
    if (d_prof)
        SFE_HIP(ctx, hipMemsetAsync(d_prof, 0, sizeof(long long) * SFE_ICP_PROF_N, ctx->stream));
    SFE_HIP(ctx, hipEventRecord(ctx->ev_loop_begin, ctx->stream)); // (where the next batch's preparation may start)
    SweepLaunchArgs a;
    a.ctx = ctx;
    a.p = p;
    a.d_jobs = d_jobs;
    a.d_src = (const float2 *)d_src;
    a.d_guess9 = d_guess9;
    a.d_stgt = d_stgt;
    a.d_perm = d_perm;
    a.d_snrm = d_snrm;
    a.d_mean = d_mean;
    a.d_tab = d_tab;
    a.d_grid = d_grid;
    a.d_qst = d_qst;
    a.d_qwl = d_qwl;
    a.d_qrsrc = d_qrsrc;
    a.d_qslot = d_qslot;
    a.d_nn_d2 = d_nn_d2;
    a.d_nn_pos = d_nn_pos;
    a.d_T9 = d_T9;
    a.d_status = d_status;
    a.d_iters = d_iters;
    a.d_prof = d_prof;
    a.d_dbg = d_dbg;
    a.sw_budget = tu.sw_budget;
    a.sw_budget_a = tu.sw_budget_a;
    a.sw_cache = pl.sw_cache;
    a.sw_cache2 = pl.sw_cache2;
    // margin of the clearance records: a search looks this fraction further (in radius) than it has to ...
    a.sw_m = 0.01f * (float)tu.sw_recm;
    // ... plus sw_kappa x the largest movement of the last step (the steps shrink geometrically once ICP converges: a
    // few times the last one covers all that are still to come)
    a.sw_kappa = tu.sw_reck;
    a.d_sync = d_sync;
    a.ox = call.ox;
    for (int i = pl.n_prep_launches; i < pl.n_launches; ++i) { // tiny, then the loop classes
        const SweepLaunch &L = pl.launches[i];
        int rc = 0;
        if (L.kind == SW_LAUNCH_TINY) {
            rc = sweep_launch_tiny(ctx, p, L.n, d_jobs, d_ids + L.id_off, d_preps, (const float2 *)d_src, (const float2 *)d_tgt, d_guess9,
                                   (const int *)d_perm, (const float2 *)d_snrm, (const float *)d_mean, (const StripTab *)d_tab, d_T9,
                                   d_status, d_iters, L.t_cap, L.q_cap, call.ox);
        } else if (L.loop.multi) { // (the shares read their gathered clouds)
            SweepLaunchArgs am = a;
            am.d_src = d_gsrc;
            rc = sweep_dispatch_loop(L.loop, am, L.n, d_ids + L.id_off, L.body, L.t_cap, L.q_cap);
        } else {
            rc = sweep_dispatch_loop(L.loop, a, L.n, d_ids + L.id_off, L.body, L.t_cap, L.q_cap);
        }
        if (rc)
            return rc;
    }
    // (recorded without bit 3 too: the next batch may come with the bit set, its preparation on the side stream)
    SFE_HIP(ctx, hipEventRecord(ctx->ev_loop[gen.g], ctx->stream));
    sfe_icp_gen_end(ctx->icp_gens, gen, side, n_split > 0);
    if (debug) {
        int h[8];
        SFE_HIP(ctx, hipMemcpyAsync(h, d_dbg, sizeof h, hipMemcpyDeviceToHost, ctx->stream));
        SFE_HIP(ctx, hipStreamSynchronize(ctx->stream));
        for (int i = 0; i < 8; ++i)
            if (h[i])
                fprintf(stderr, "sfe_icp_sweep: watchdog %d tripped (workgroup %d)\n", i, h[i] - 1);
    }
    if (d_prof) {
        SFE_HIP(ctx, hipMemcpyAsync(ctx->icp_prof_host, d_prof, sizeof(long long) * SFE_ICP_PROF_N, hipMemcpyDeviceToHost,
                                    ctx->stream));
        SFE_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    return 0;
}

extern "C" int sfe_icp_last_routes(sfe_ctx *ctx, int32_t *route, int n_jobs, int32_t *n_cu)
{
    if (!ctx)
        return SFE_ERR_ARG;
    SFE_ARG(ctx, n_jobs >= 0 && (route || n_jobs == 0) && (n_jobs == 0 || n_jobs == (int)ctx->icp_routes.size()));
    for (int j = 0; j < n_jobs; ++j)
        route[j] = ctx->icp_routes[(size_t)j];
    if (n_cu)
        *n_cu = ctx->n_cu;
    return 0;
}

extern "C" int sfe_icp_get_profile(sfe_ctx *ctx, int enable, long long *cycles16)
{
    if (!ctx)
        return SFE_ERR_ARG;
    if (cycles16)
        for (int i = 0; i < SFE_ICP_PROF_N; ++i)
            cycles16[i] = ctx->icp_prof_host[i];
    ctx->icp_prof = enable;
    return 0;
}
