// Strip-sweep ICP, host side: which copy ("generation") of the prepared-target scratch a batch uses, and which earlier
// loop kernels its preparation has to wait for.  Plain C++ (no HIP), so that the rules can be run on their own
// (tests/host/icp_gen_check.cpp).
//
// Under sfe_icp_set_tuning bit 3 the preparation of a batch (job tables, sorted targets, normals, strip tables, witness
// grids) is enqueued on the side stream and its loop kernels on the main stream, behind it.  With ONE copy of what the
// preparation writes, the preparation of batch k+1 must wait for the loop of batch k.  With two copies, used in turn, it
// waits for the loop that last read ITS copy -- two batches back -- and runs beside the loop kernel of batch k.
//   * Without bit 3 a batch uses generation 0 and everything is enqueued on the main stream, where it is behind every
//     earlier loop kernel anyway (they all run on the main stream), whichever generation those read.
//   * The scratch of jobs shared by several workgroups (gathered clouds, sync areas) exists once: a preparation that
//     writes it waits for the newest loop kernel, i.e. for all of them.
//   * The shares of a shared job must all be resident at the same time (SFE_ICP_SPLIT_TIMEOUT), so no later
//     preparation may take CUs while such a loop kernel runs: the first side-stream preparation enqueued behind one
//     waits for the newest loop kernel as well.
#pragma once

struct SfeIcpGenState {
    unsigned n_side = 0;             // batches enqueued under bit 3 so far
    bool pending[2] = {false, false}; // ev_loop[g] has been recorded behind a loop that reads generation g
    int newest = -1;                 // generation of the loop enqueued last (its event is behind every earlier loop)
    bool shared_unwaited = false;    // a loop with shared jobs was enqueued and no preparation has waited for it yet
    // sfe_icp_gen_begin was called and sfe_icp_gen_end was not: a launch gave up half-way, with an error, and what it had
    // enqueued by then (waits, preparation kernels, some loop kernels without their event) is not in this state
    bool open = false;
};

struct SfeIcpGenPlan {
    int g;        // generation of this batch
    bool wait[2]; // the preparation stream waits for ev_loop[0] / ev_loop[1] first
    // ... and for the point where the newest batch's loop kernels begin (ev_loop_begin): the preparation is meant to take
    // workgroup slots beside a long loop kernel (DESIGN.md 5.3 has the trace), not to compete with whatever the caller enqueued in
    // front of that loop kernel (a batch pipeline's front end: short kernels, between which a low priority counts for
    // nothing).  It still has that whole loop kernel's time to finish before its own loop kernels are due.
    bool wait_begin;
    // the launch before ended with an error between begin and end: wait on the host for both streams before anything else
    // (the state has been reset to "nothing pending", which is true once they are idle)
    bool sync_first;
    bool waits_shared; // wait[] covers a loop with shared jobs: sfe_icp_gen_end notes that it has been waited for
};

// side: bit 3 is set for this batch; has_shared: it holds jobs shared by several workgroups.  Apart from `open` (and the
// reset that goes with sync_first) the state only changes in sfe_icp_gen_end, i.e. once everything the plan asks for
// has been enqueued: a launch that returns an error in between leaves no wait noted that was never enqueued.
static inline SfeIcpGenPlan sfe_icp_gen_begin(SfeIcpGenState &s, bool side, bool has_shared)
{
    SfeIcpGenPlan pl;
    pl.sync_first = s.open;
    pl.waits_shared = false;
    if (s.open) {
        s.pending[0] = s.pending[1] = false;
        s.newest = -1;
        s.shared_unwaited = false;
    }
    s.open = true;
    pl.g = side ? (int)(s.n_side & 1u) : 0;
    pl.wait[0] = pl.wait[1] = false;
    pl.wait_begin = side && s.newest >= 0;
    if (!side)
        return pl; // stream order does it
    pl.wait[pl.g] = s.pending[pl.g];
    if ((has_shared || s.shared_unwaited) && s.newest >= 0) {
        pl.wait[s.newest] = true;
        pl.waits_shared = true; // (whatever the side stream takes later is behind this wait)
    }
    return pl;
}

// the loop kernels of the batch have been enqueued and ev_loop[pl.g] recorded behind them
static inline void sfe_icp_gen_end(SfeIcpGenState &s, const SfeIcpGenPlan &pl, bool side, bool has_shared)
{
    s.open = false;
    s.pending[pl.g] = true;
    s.newest = pl.g;
    if (pl.waits_shared)
        s.shared_unwaited = false;
    if (has_shared)
        s.shared_unwaited = true;
    if (side)
        ++s.n_side;
}
