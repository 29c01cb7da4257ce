// CPU check of the 3-D keyframe store's host-side bookkeeping (sonar_slam_amd/csrc/sfe_store3_slots.h): reserve, compact
// placement, truncate and the overflow tests, against a model that keeps a plain list of (offset, count).
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Wall -Wextra -Werror
//       tests/host/store3_slots_check.cpp -o store3_slots_check && ./store3_slots_check
//
// Covered: exact fill of the pool and of the slot table; overflow by one point and by one slot (nothing changes); truncate
// to 0, to the current count and beyond it; offsets and sizes above 2^31; get_points' reserve-then-place (an upper bound is
// tested, the real sizes are placed one behind the other); a random walk of pushes and truncates against the model.
#include "../../sonar_slam_amd/csrc/sfe_store3_slots.h"

#include <cstdio>
#include <cstdlib>
#include <utility>

static int g_fail = 0;
#define CHECK(cond)                                                            \
    do {                                                                       \
        if (!(cond)) {                                                         \
            printf("FAILED %s (line %d)\n", #cond, __LINE__);                  \
            ++g_fail;                                                          \
        }                                                                      \
    } while (0)

struct Snapshot {
    int64_t top;
    int32_t n;
    std::vector<int64_t> off, cnt, stamp;
};

static Snapshot snap(const Store3Slots &t)
{
    Snapshot s{t.top, t.n_slots, {}, {}, {}};
    for (int32_t i = 0; i < t.n_slots; ++i) {
        s.off.push_back(t.off[(size_t)i]);
        s.cnt.push_back(t.cnt[(size_t)i]);
        s.stamp.push_back(t.stamp[(size_t)i]);
    }
    return s;
}

static bool same(const Snapshot &a, const Snapshot &b)
{
    return a.top == b.top && a.n == b.n && a.off == b.off && a.cnt == b.cnt && a.stamp == b.stamp;
}

// every slot begins where the one before it ends, and the fill level is the end of the last
static void check_compact(const Store3Slots &t)
{
    int64_t at = 0;
    for (int32_t i = 0; i < t.n_slots; ++i) {
        CHECK(t.off[(size_t)i] == at);
        CHECK(t.cnt[(size_t)i] >= 0);
        at += t.cnt[(size_t)i];
    }
    CHECK(t.top == at);
    CHECK(t.top <= t.capacity && t.n_slots <= t.max_clouds);
}

static void exact_fill_and_overflow()
{
    Store3Slots t;
    t.init(1000, 4);
    CHECK(t.push(7, 600) == 0);
    const Snapshot before = snap(t);
    CHECK(!t.fits(401, 1)); // one point too many
    CHECK(t.push(8, 401) == -1);
    CHECK(t.push(8, 600) == -1);
    CHECK(same(before, snap(t)));
    CHECK(t.fits(400, 1));
    CHECK(t.push(9, 400) == 1); // exact fill of the pool
    CHECK(t.top == 1000 && t.off[1] == 600 && t.cnt[1] == 400 && t.stamp[1] == 9);
    CHECK(!t.fits(1, 1) && t.fits(0, 1));
    CHECK(t.push(0, 1) == -1);
    CHECK(t.push(10, 0) == 2 && t.push(11, 0) == 3); // empty slots: exact fill of the slot table
    const Snapshot full = snap(t);
    CHECK(!t.fits(0, 1)); // one slot too many
    CHECK(t.push(12, 0) == -1);
    CHECK(same(full, snap(t)));
    CHECK(!t.fits(-1, 1) && !t.fits(0, -1));
    check_compact(t);
}

static void truncates()
{
    Store3Slots t;
    t.init(100, 8);
    for (int i = 0; i < 5; ++i)
        CHECK(t.push(i, 10 + i) == i);
    const Snapshot s5 = snap(t);
    CHECK(t.truncate(5) && same(s5, snap(t))); // to the current count: nothing moves
    CHECK(!t.truncate(6) && !t.truncate(-1) && same(s5, snap(t)));
    CHECK(t.truncate(3) && t.n_slots == 3 && t.top == 10 + 11 + 12);
    CHECK(t.push(50, 1) == 3 && t.off[3] == 33); // the handle and the pool are reused
    CHECK(t.truncate(0) && t.n_slots == 0 && t.top == 0);
    CHECK(t.truncate(0));
    CHECK(t.push(1, 100) == 0 && t.off[0] == 0);
    // a released empty slot at the end
    CHECK(t.truncate(0) && t.push(1, 40) == 0 && t.push(2, 0) == 1 && t.truncate(1) && t.top == 40);
    check_compact(t);
}

static void beyond_2_31()
{
    Store3Slots t;
    const int64_t big = (int64_t)1 << 28; // the largest single cloud
    t.init(((int64_t)1 << 33) + 5, 64);
    for (int i = 0; i < 32; ++i)
        CHECK(t.push(i, big) == i);
    CHECK(t.top == (int64_t)1 << 33 && t.off[31] == 31 * big && t.off[31] > ((int64_t)1 << 31));
    CHECK(t.fits(5, 1) && !t.fits(6, 1));
    CHECK(!t.fits(INT64_MAX, 1) && !t.fits(5, INT64_MAX)); // (no sum is formed that could overflow)
    CHECK(t.push(99, 5) == 32 && t.off[32] == (int64_t)1 << 33);
    CHECK(t.truncate(20) && t.top == 20 * big);
    check_compact(t);
}

// get_points: the call tests an upper bound (the sum of its input counts, its number of jobs), then places the real sizes
static void reserve_then_place()
{
    Store3Slots t;
    t.init(1000, 6);
    CHECK(t.push(0, 300) == 0 && t.push(1, 200) == 1);
    const Snapshot before = snap(t);
    const int64_t bound_ok[3] = {300, 200, 0}, real[3] = {120, 77, 0};
    CHECK(t.fits(bound_ok[0] + bound_ok[1] + bound_ok[2], 3));
    for (int j = 0; j < 3; ++j)
        CHECK(t.push(10 + j, real[j]) == 2 + j);
    CHECK(t.off[2] == 500 && t.off[3] == 620 && t.off[4] == 697 && t.top == 697); // right behind, not behind the bound
    CHECK(t.truncate(2) && same(before, snap(t)));
    CHECK(!t.fits(501, 1)); // a bound that does not fit: the call stops here
    CHECK(!t.fits(10, 5));  // ... or its jobs do not
    CHECK(same(before, snap(t)));
    check_compact(t);
}

static void random_walk()
{
    unsigned long long x = 88172645463325252ull;
    auto rnd = [&x]() {
        x ^= x << 13;
        x ^= x >> 7;
        x ^= x << 17;
        return x;
    };
    Store3Slots t;
    t.init(5000, 40);
    std::vector<std::pair<int64_t, int64_t>> model; // (offset, count)
    int64_t top = 0;
    for (int step = 0; step < 20000; ++step) {
        if (rnd() % 4 != 0) {
            const int64_t n = (int64_t)(rnd() % 700);
            const bool room = top + n <= 5000 && model.size() < 40;
            CHECK(t.fits(n, 1) == room);
            const int32_t h = t.push(step, n);
            if (room) {
                CHECK(h == (int32_t)model.size());
                model.push_back({top, n});
                top += n;
            } else {
                CHECK(h == -1);
            }
        } else {
            const int64_t keep = (int64_t)(rnd() % (model.size() + 2));
            const bool ok = keep <= (int64_t)model.size();
            CHECK(t.truncate(keep) == ok);
            if (ok && keep < (int64_t)model.size()) {
                top = model[(size_t)keep].first;
                model.resize((size_t)keep);
            }
        }
        CHECK(t.n_slots == (int32_t)model.size() && t.top == top);
        for (size_t i = 0; i < model.size(); ++i)
            CHECK(t.off[i] == model[i].first && t.cnt[i] == model[i].second);
        CHECK(t.valid(-1) == false && t.valid(t.n_slots) == false && (t.n_slots == 0 || t.valid(t.n_slots - 1)));
        if (g_fail)
            return;
    }
    check_compact(t);
}

int main()
{
    exact_fill_and_overflow();
    truncates();
    beyond_2_31();
    reserve_then_place();
    random_walk();
    if (g_fail) {
        printf("store3_slots_check: %d failures\n", g_fail);
        return 1;
    }
    printf("store3_slots_check: ok\n");
    return 0;
}
