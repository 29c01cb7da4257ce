// Stand-alone check of the generation rules of the strip-sweep ICP launcher (sonar_slam_amd/csrc/sfe_icp_gen.h), run on
// the CPU: every sequence of up to 9 batches, each with or without sfe_icp_set_tuning bit 3 and with or without jobs
// shared by several workgroups, against a model of the two streams.  tests/test_icp_gen_rules.py builds it plainly; under
// the sanitizers it is a program of its own (no GPU, nothing preloaded):
//   g++ -std=c++17 -O1 -g -Wall -Wextra -Werror -fsanitize=address,undefined -fno-sanitize-recover=all
//       tests/host/icp_gen_check.cpp -o icp_gen_check && ./icp_gen_check
//
// Model: the loop kernels of batch i run on the main stream, in order; ev_loop[g] is recorded behind them, so waiting for
// the event that batch m recorded covers the loops of every batch <= m.  The side stream is in order as well: what one
// preparation has waited for, every later one is behind too (`covered` = the newest batch the side stream is behind).
// A batch without bit 3 is enqueued on the main stream and is behind every earlier loop.
// A launch may also give up with an error between sfe_icp_gen_begin and sfe_icp_gen_end (sequences of up to 6): whatever
// it enqueued is behind no event, so the next launch must be told to wait for both streams on the host, and starts from
// an idle context.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../sonar_slam_amd/csrc/sfe_icp_gen.h"

struct Batch {
    bool side, shared;
    int g;
};

static long long g_checked = 0;

#define CHECK(cond)                                                                                   \
    do {                                                                                              \
        if (!(cond)) {                                                                                \
            std::fprintf(stderr, "icp_gen_check: %s fails (line %d), sequence:", #cond, __LINE__);   \
            for (const Batch &b : seq)                                                                \
                std::fprintf(stderr, " %s%s/g%d", b.side ? "side" : "main", b.shared ? "+shared" : "", b.g); \
            std::fprintf(stderr, "\n");                                                               \
            std::exit(1);                                                                             \
        }                                                                                             \
    } while (0)

static void run(const std::vector<int> &kinds)
{
    SfeIcpGenState st;
    std::vector<Batch> seq;
    int ev[2] = {-1, -1}; // the batch whose loops ev_loop[g] stands behind
    int covered = -1;
    for (size_t i = 0; i < kinds.size(); ++i) {
        const bool side = (kinds[i] & 1) != 0, shared = (kinds[i] & 2) != 0, fails = (kinds[i] & 4) != 0;
        const bool after_failure = i > 0 && (kinds[i - 1] & 4) != 0;
        const SfeIcpGenPlan pl = sfe_icp_gen_begin(st, side, shared);
        seq.push_back({side, shared, pl.g});
        CHECK(pl.sync_first == after_failure);
        if (pl.sync_first) { // the host has waited for both streams: every earlier batch is done, no event counts
            covered = (int)i - 1;
            ev[0] = ev[1] = -1;
            CHECK(!pl.wait[0] && !pl.wait[1] && !pl.wait_begin);
        }
        CHECK(pl.g == 0 || pl.g == 1);
        CHECK(side || pl.g == 0);
        CHECK(side || (!pl.wait[0] && !pl.wait[1] && !pl.wait_begin));
        CHECK(!side || pl.wait_begin == (i > 0 && !after_failure)); // behind the point where the batch before began its loop kernels
        for (int g = 0; g < 2; ++g)
            if (pl.wait[g]) {
                CHECK(ev[g] >= 0); // never waits for an event that was not recorded
                if (ev[g] > covered)
                    covered = ev[g];
            }
        if (side) {
            for (size_t j = 0; j < i; ++j) {
                // the preparation rewrites generation g: no earlier loop that reads it may be running
                if (seq[j].g == pl.g)
                    CHECK((int)j <= covered);
                // the shares of a shared job are resident together: no preparation next to such a loop
                if (seq[j].shared)
                    CHECK((int)j <= covered);
                // the scratch of shared jobs exists once: a preparation that writes it is behind every loop
                if (shared)
                    CHECK((int)j <= covered);
            }
            // the point of two generations: with bit 3 on both and no shared jobs in sight, the preparation
            // does not wait for the batch right before it
            if (i > 0 && seq[i - 1].side && !shared && !after_failure) {
                bool any_shared = false;
                for (size_t j = 0; j < i; ++j)
                    any_shared = any_shared || seq[j].shared;
                if (!any_shared)
                    CHECK(covered < (int)i - 1);
            }
        }
        // consecutive batches under bit 3 alternate
        if (i > 0 && side && seq[i - 1].side && !after_failure)
            CHECK(pl.g != seq[i - 1].g);
        ++g_checked;
        if (fails)
            continue; // no sfe_icp_gen_end, no event
        sfe_icp_gen_end(st, pl, side, shared);
        ev[pl.g] = (int)i;
    }
}

static void sequences(int max_len, int n_kinds)
{
    for (int len = 1; len <= max_len; ++len) {
        std::vector<int> kinds((size_t)len, 0);
        for (;;) {
            run(kinds);
            int k = 0;
            while (k < len && ++kinds[(size_t)k] == n_kinds)
                kinds[(size_t)k++] = 0;
            if (k == len)
                break;
        }
    }
}

int main()
{
    sequences(9, 4);
    sequences(6, 8); // ... with launches that fail
    std::printf("icp_gen_check: ok, %lld batches checked\n", g_checked);
    return 0;
}
