// CPU check of the keyed-cloud bookkeeping of the 3-D keyframe store (sonar_slam_amd/csrc/sfe_store3_slots.h): the per-slot
// flags, the upper bounds the keyed calls hand to fits(), and the job table of get_points / get_points_keys.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Wall -Wextra -Werror
//       tests/host/store3_keys_check.cpp -o store3_keys_check && ./store3_keys_check
//
// Covered: the keyed and selected flags across push and truncate, a re-push over a released keyed slot (plain again, no
// selection); the bounds of put_keys, get_points_keys and compact_selected, with a call that fits exactly and one that is one
// point or one slot too large (nothing changes); the job table: unused (-1) and empty entries leave no segment, dst offsets,
// per-job and overall totals, keys per segment, jobs without entries, unknown handles, negative keys (looked at only where
// the entry leaves a segment), offsets that run backwards, a concatenation beyond 2^28 points.
#include "../../sonar_slam_amd/csrc/sfe_store3_slots.h"

#include <cstdio>
#include <cstdlib>

static int g_fail = 0;
#define CHECK(cond)                                                            \
    do {                                                                       \
        if (!(cond)) {                                                         \
            printf("FAILED %s (line %d)\n", #cond, __LINE__);                  \
            ++g_fail;                                                          \
        }                                                                      \
    } while (0)

static void flags()
{
    Store3Slots t;
    t.init(1000, 8);
    CHECK(t.push(1, 100) == 0);            // the two-argument form stays: a plain slot
    CHECK(t.push(2, 50, true) == 1);
    CHECK(t.push(3, 0, true) == 2);        // an empty keyed slot
    CHECK(t.push(4, 10, false) == 3);
    CHECK(!t.is_keyed(0) && t.is_keyed(1) && t.is_keyed(2) && !t.is_keyed(3));
    CHECK(!t.is_keyed(-1) && !t.is_keyed(4) && !t.has_selection(-1) && !t.has_selection(4));
    for (int h = 0; h < 4; ++h)
        CHECK(!t.has_selection(h));
    t.selected[1] = 1;                     // what fov_select / set_selection record
    t.selected[2] = 1;
    CHECK(t.has_selection(1) && t.has_selection(2) && !t.has_selection(3));
    // truncate to the current count changes nothing
    CHECK(t.truncate(4) && t.is_keyed(1) && t.has_selection(1));
    // release slots 1 .. 3; a re-push over the released keyed slot is plain and has no selection
    CHECK(t.truncate(1) && t.n_slots == 1 && t.top == 100);
    CHECK(!t.is_keyed(1) && !t.has_selection(1));
    CHECK(t.keyed[1] == 0 && t.selected[1] == 0 && t.keyed[2] == 0 && t.selected[2] == 0);
    CHECK(t.push(5, 20) == 1 && !t.is_keyed(1) && !t.has_selection(1));
    // ... even when the flags were set behind the table's back (push itself clears them)
    t.keyed[2] = 1;
    t.selected[2] = 1;
    CHECK(t.push(6, 5) == 2 && !t.is_keyed(2) && !t.has_selection(2));
    CHECK(t.push(7, 5, true) == 3 && t.is_keyed(3) && !t.has_selection(3));
    // a refused push changes no flag
    t.selected[3] = 1;
    CHECK(t.push(8, 5000, true) == -1 && t.n_slots == 4 && t.is_keyed(3) && t.has_selection(3));
    CHECK(!t.truncate(5) && t.is_keyed(3) && t.has_selection(3));
    CHECK(t.truncate(0) && !t.is_keyed(0) && t.keyed[3] == 0 && t.selected[3] == 0);
}

static void bounds()
{
    Store3Slots t;
    t.init(1000, 5);
    CHECK(t.push(0, 300, true) == 0 && t.push(1, 200, true) == 1 && t.push(2, 0, true) == 2);
    // put_keys: the cloud itself, one slot
    S3Bound b = s3_bound_put(500);
    CHECK(b.points == 500 && b.slots == 1 && t.fits(b.points, b.slots));
    b = s3_bound_put(501);
    CHECK(!t.fits(b.points, b.slots));
    // compact_selected: the sum of the clouds' counts (a cloud named twice counts twice), n_jobs slots
    const int32_t twice[2] = {0, 1};
    b = s3_bound_compact(t, twice, 2);
    CHECK(b.points == 500 && b.slots == 2 && t.fits(b.points, b.slots)); // exactly the room that is left
    const int32_t thrice[3] = {0, 1, 2};
    b = s3_bound_compact(t, thrice, 3);
    CHECK(b.points == 500 && b.slots == 3 && !t.fits(b.points, b.slots)); // one slot too many
    const int32_t dup[2] = {0, 0};
    b = s3_bound_compact(t, dup, 2);
    CHECK(b.points == 600 && !t.fits(b.points, b.slots)); // points
    b = s3_bound_compact(t, dup, 0);
    CHECK(b.points == 0 && b.slots == 0 && t.fits(b.points, b.slots));
    // get_points_keys: the sum of the concatenations, n_jobs slots
    const float H[12 * 3] = {0};
    const int32_t handles[3] = {0, 1, 1}, keys[3] = {4, 5, 6};
    const int64_t off2[3] = {0, 2, 3};
    S3JobTable tab;
    int bj = -1;
    int64_t be = -1;
    CHECK(s3_build_jobs(t, handles, H, keys, off2, 2, tab, &bj, &be) == S3_JOBS_OK);
    b = s3_bound_get_points(tab);
    CHECK(b.points == 700 && b.slots == 2 && !t.fits(b.points, b.slots));
    const int64_t off1[2] = {0, 2};
    CHECK(s3_build_jobs(t, handles, H, keys, off1, 1, tab, &bj, &be) == S3_JOBS_OK);
    b = s3_bound_get_points(tab);
    CHECK(b.points == 500 && b.slots == 1 && t.fits(b.points, b.slots));
    CHECK(t.n_slots == 3 && t.top == 500); // (asking changes nothing)
}

static void job_table()
{
    Store3Slots t;
    t.init(100000, 16);
    const int64_t sizes[6] = {10, 0, 7, 300, 0, 25};
    for (int i = 0; i < 6; ++i)
        CHECK(t.push(i, sizes[i], i % 2 == 0) == i);
    // job 0: [0, -1, 1 (empty), 2]   job 1: []   job 2: [-1]   job 3: [3, 3, 5]   job 4: [4 (empty)]
    const int32_t handles[9] = {0, -1, 1, 2, -1, 3, 3, 5, 4};
    const int32_t keys[9] = {11, -7 /* unused entry: not looked at */, -8 /* empty cloud: not looked at */, 13, 14, 15, 16, 17, 18};
    const int64_t off[6] = {0, 4, 4, 5, 8, 9};
    float H[12 * 9];
    for (int i = 0; i < 12 * 9; ++i)
        H[i] = (float)i;
    S3JobTable tab;
    int bj = -1;
    int64_t be = -1;
    CHECK(s3_build_jobs(t, handles, H, keys, off, 5, tab, &bj, &be) == S3_JOBS_OK);
    CHECK(tab.jobs.size() == 5 && tab.segs.size() == 5 && tab.seg_key.size() == 5);
    CHECK(tab.total == 10 + 7 + 300 + 300 + 25 && tab.max_tot == 625);
    const S3Job *J = tab.jobs.data();
    CHECK(J[0].cat == 0 && J[0].tot == 17 && J[0].seg0 == 0 && J[0].nseg == 2);
    CHECK(J[1].cat == 17 && J[1].tot == 0 && J[1].seg0 == 2 && J[1].nseg == 0);
    CHECK(J[2].cat == 17 && J[2].tot == 0 && J[2].seg0 == 2 && J[2].nseg == 0);
    CHECK(J[3].cat == 17 && J[3].tot == 625 && J[3].seg0 == 2 && J[3].nseg == 3);
    CHECK(J[4].cat == 642 && J[4].tot == 0 && J[4].seg0 == 5 && J[4].nseg == 0);
    const S3Seg *g = tab.segs.data();
    CHECK(g[0].src == 0 && g[0].n == 10 && g[0].dst == 0 && g[0].H[0] == 0.0f && g[0].H[11] == 11.0f);
    CHECK(g[1].src == 10 && g[1].n == 7 && g[1].dst == 10 && g[1].H[0] == 36.0f); // entry 3's transform
    CHECK(g[2].src == 17 && g[2].n == 300 && g[2].dst == 0 && g[2].H[0] == 60.0f);
    CHECK(g[3].src == 17 && g[3].n == 300 && g[3].dst == 300 && g[3].H[0] == 72.0f);
    CHECK(g[4].src == 317 && g[4].n == 25 && g[4].dst == 600 && g[4].H[11] == 95.0f);
    const int32_t want_keys[5] = {11, 13, 15, 16, 17};
    for (int i = 0; i < 5; ++i)
        CHECK(tab.seg_key[(size_t)i] == want_keys[i]);
    // every segment lies inside its job's concatenation and the segments of a job tile it
    for (const S3Job &j : tab.jobs) {
        int at = 0;
        for (int k = 0; k < j.nseg; ++k) {
            CHECK(tab.segs[(size_t)(j.seg0 + k)].dst == at && tab.segs[(size_t)(j.seg0 + k)].n > 0);
            at += tab.segs[(size_t)(j.seg0 + k)].n;
        }
        CHECK(at == j.tot);
    }
    // without keys (get_points): the same table, no key list
    CHECK(s3_build_jobs(t, handles, H, nullptr, off, 5, tab, &bj, &be) == S3_JOBS_OK);
    CHECK(tab.segs.size() == 5 && tab.seg_key.empty() && tab.total == 642);
    // no jobs at all
    CHECK(s3_build_jobs(t, handles, H, keys, off, 0, tab, &bj, &be) == S3_JOBS_OK);
    CHECK(tab.jobs.empty() && tab.segs.empty() && tab.total == 0 && tab.max_tot == 0);

    // refusals: which job and which entry
    int32_t bad_h[9];
    for (int i = 0; i < 9; ++i)
        bad_h[i] = handles[i];
    bad_h[6] = 6; // the store holds 6 slots
    CHECK(s3_build_jobs(t, bad_h, H, keys, off, 5, tab, &bj, &be) == S3_JOBS_BAD_HANDLE && bj == 3 && be == 6);
    bad_h[6] = -2;
    CHECK(s3_build_jobs(t, bad_h, H, keys, off, 5, tab, &bj, &be) == S3_JOBS_BAD_HANDLE && bj == 3 && be == 6);
    int32_t bad_k[9];
    for (int i = 0; i < 9; ++i)
        bad_k[i] = keys[i];
    bad_k[7] = -1;
    CHECK(s3_build_jobs(t, handles, H, bad_k, off, 5, tab, &bj, &be) == S3_JOBS_BAD_KEY && bj == 3 && be == 7);
    CHECK(s3_build_jobs(t, handles, H, nullptr, off, 5, tab, &bj, &be) == S3_JOBS_OK);
    const int64_t back[3] = {0, 4, 3};
    CHECK(s3_build_jobs(t, handles, H, keys, back, 2, tab, &bj, &be) == S3_JOBS_BAD_OFFSETS && bj == 1);
    const int64_t neg[2] = {-1, 2};
    CHECK(s3_build_jobs(t, handles, H, keys, neg, 1, tab, &bj, &be) == S3_JOBS_BAD_OFFSETS && bj == 0);
}

static void too_many_points()
{
    Store3Slots t;
    t.init((int64_t)1 << 30, 4);
    CHECK(t.push(0, (int64_t)1 << 28) == 0 && t.push(1, 1) == 1);
    const int32_t handles[2] = {0, 1}, keys[2] = {0, 0};
    const float H[24] = {0};
    const int64_t off[2] = {0, 2}, off_one[2] = {0, 1};
    S3JobTable tab;
    int bj = -1;
    int64_t be = -1;
    CHECK(s3_build_jobs(t, handles, H, keys, off_one, 1, tab, &bj, &be) == S3_JOBS_OK && tab.max_tot == S3_MAX_POINTS);
    CHECK(s3_build_jobs(t, handles, H, keys, off, 1, tab, &bj, &be) == S3_JOBS_TOO_MANY_POINTS && bj == 0 && be == 1);
}

int main()
{
    flags();
    bounds();
    job_table();
    too_many_points();
    if (g_fail) {
        printf("store3_keys_check: %d failures\n", g_fail);
        return 1;
    }
    printf("store3_keys_check: ok\n");
    return 0;
}
