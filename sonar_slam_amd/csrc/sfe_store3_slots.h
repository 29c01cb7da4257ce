// Host-side bookkeeping of the 3-D keyframe store (sfe_store3.hip): the slot table, the pool's fill level and the job table of
// get_points / get_points_keys.  Plain C++ without a HIP call, so that tests/host/store3_slots_check.cpp and
// tests/host/store3_keys_check.cpp can run it on the CPU under the sanitizers.
//
// A pool of `capacity` points and a table of `max_clouds` slots {stamp, offset, count}.  Clouds are packed back to back:
// slot k + 1 begins where slot k ends, so the fill level is the end of the last slot.  Handles (slot indices) are handed out
// in order and released in stack order.  Every size is an int64: a pool may hold more than 2^31 points.
//
//   fits(points, slots)  would `slots` more clouds of `points` points in all still fit?  (the test a call makes BEFORE it
//                        launches anything: put with the cloud's size, get_points with the sum of its input counts -- an
//                        upper bound of what the downsample leaves)
//   push(stamp, n)       the next slot, placed at the fill level -> its handle; the caller has asked fits() first, for the
//                        size itself or for an upper bound of it: placing the real sizes one behind the other is the compact
//                        placement of get_points
//   truncate(n_slots)    releases every slot at or above n_slots and the pool behind them
//
// Two flags per slot: `keyed` (the key pool holds a key per point of the cloud: push's third argument) and `selected` (the
// selection pool holds a byte per point of it: fov_select or set_selection wrote one).  push and truncate clear both, so a
// slot handed out again never inherits them.
//
// The upper bounds the keyed calls hand to fits() (s3_bound_*): each is the largest result the call can leave, in points
// and in slots, so that nothing can turn out not to fit after the launch.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

struct Store3Slots {
    int64_t capacity = 0;   // points
    int64_t top = 0;        // points in use = offset of the next cloud
    int32_t max_clouds = 0;
    int32_t n_slots = 0;    // slots in use = the next handle
    std::vector<int64_t> stamp, off, cnt;
    std::vector<uint8_t> keyed, selected;

    void init(int64_t capacity_points, int32_t max_clouds_)
    {
        capacity = capacity_points;
        max_clouds = max_clouds_;
        top = 0;
        n_slots = 0;
        stamp.assign((size_t)max_clouds_, 0);
        off.assign((size_t)max_clouds_, 0);
        cnt.assign((size_t)max_clouds_, 0);
        keyed.assign((size_t)max_clouds_, 0);
        selected.assign((size_t)max_clouds_, 0);
    }

    // (written as differences: capacity - top and max_clouds - n_slots cannot overflow, a sum of the arguments could)
    bool fits(int64_t points, int64_t slots) const
    {
        return points >= 0 && slots >= 0 && points <= capacity - top && slots <= (int64_t)max_clouds - (int64_t)n_slots;
    }

    bool valid(int64_t handle) const { return handle >= 0 && handle < (int64_t)n_slots; }
    bool is_keyed(int64_t handle) const { return valid(handle) && keyed[(size_t)handle] != 0; }
    bool has_selection(int64_t handle) const { return valid(handle) && selected[(size_t)handle] != 0; }

    // -> the new handle, or -1 if the cloud does not fit (nothing changes then)
    int32_t push(int64_t stamp_, int64_t n, bool keyed_ = false)
    {
        if (!fits(n, 1))
            return -1;
        const int32_t h = n_slots;
        stamp[(size_t)h] = stamp_;
        off[(size_t)h] = top;
        cnt[(size_t)h] = n;
        keyed[(size_t)h] = keyed_ ? 1 : 0;
        selected[(size_t)h] = 0;
        top += n;
        ++n_slots;
        return h;
    }

    // -> false (nothing changes) unless 0 <= n <= n_slots
    bool truncate(int64_t n)
    {
        if (n < 0 || n > (int64_t)n_slots)
            return false;
        if (n < (int64_t)n_slots) {
            for (int64_t h = n; h < (int64_t)n_slots; ++h)
                keyed[(size_t)h] = selected[(size_t)h] = 0;
            top = off[(size_t)n]; // where the first released cloud began
            n_slots = (int32_t)n;
        }
        return true;
    }
};

// ---- the job table of get_points and get_points_keys -------------------------------------------------------------------------
#define S3_MAX_POINTS (1 << 28) // largest cloud / concatenation: the kernels index a cloud's points with an int

struct S3Seg { // one input cloud of a get_points job
    long long src; // its first point in the pool
    int n;         // its points (> 0: empty and unused entries are dropped on the host)
    int dst;       // its first point in the job's concatenation
    float H[12];   // rows 0..2 of the 4 x 4 transform
};

struct S3Job { // one get_points job
    long long cat; // first point of its concatenation in the scratch arrays
    int tot;       // points of the concatenation
    int seg0, nseg; // its segments
    int pad;
};

struct S3JobTable {
    std::vector<S3Job> jobs;
    std::vector<S3Seg> segs;
    std::vector<int32_t> seg_key; // one per segment (only with keys)
    int64_t total = 0;            // points of all concatenations = the call's upper bound
    int max_tot = 0;              // the largest concatenation
};

enum { S3_JOBS_OK = 0, S3_JOBS_BAD_HANDLE = 1, S3_JOBS_TOO_MANY_POINTS = 2, S3_JOBS_BAD_KEY = 3, S3_JOBS_BAD_OFFSETS = 4 };

// Job j lists the entries [job_off[j], job_off[j + 1]) of handles / H12 (12 floats each) / keys (nullable: no keys).  An
// entry of -1 is unused; an unused entry and an empty cloud leave no segment (their key is not looked at).  -> S3_JOBS_OK, or
// the reason with *bad_job and *bad_entry set (the table's contents are then unspecified).
inline int s3_build_jobs(const Store3Slots &t, const int32_t *handles, const float *H12, const int32_t *keys,
                         const int64_t *job_off, int n_jobs, S3JobTable &out, int *bad_job, int64_t *bad_entry)
{
    out.jobs.assign((size_t)n_jobs, S3Job{0, 0, 0, 0, 0});
    out.segs.clear();
    out.seg_key.clear();
    out.total = 0;
    out.max_tot = 0;
    for (int j = 0; j < n_jobs; ++j) {
        *bad_job = j;
        *bad_entry = job_off[j];
        if (job_off[j] < 0 || job_off[j + 1] < job_off[j])
            return S3_JOBS_BAD_OFFSETS;
        int64_t tot = 0;
        const int seg0 = (int)out.segs.size();
        for (int64_t e = job_off[j]; e < job_off[j + 1]; ++e) {
            *bad_entry = e;
            const int32_t h = handles[e];
            if (h == -1)
                continue;
            if (!t.valid(h))
                return S3_JOBS_BAD_HANDLE;
            if (t.cnt[(size_t)h] == 0)
                continue;
            if (keys && keys[e] < 0)
                return S3_JOBS_BAD_KEY;
            S3Seg g;
            g.src = t.off[(size_t)h];
            g.n = (int)t.cnt[(size_t)h];
            g.dst = (int)tot;
            memcpy(g.H, H12 + 12 * (size_t)e, sizeof g.H);
            tot += g.n;
            if (tot > S3_MAX_POINTS)
                return S3_JOBS_TOO_MANY_POINTS;
            out.segs.push_back(g);
            if (keys)
                out.seg_key.push_back(keys[e]);
        }
        out.jobs[(size_t)j] = S3Job{out.total, (int)tot, seg0, (int)out.segs.size() - seg0, 0};
        out.total += tot;
        if ((int)tot > out.max_tot)
            out.max_tot = (int)tot;
    }
    return S3_JOBS_OK;
}

// ---- the upper bounds the keyed calls hand to fits(): {points, slots} ------------------------------------------------------------
struct S3Bound {
    int64_t points, slots;
};

// put_keys: the cloud itself
inline S3Bound s3_bound_put(int64_t n) { return S3Bound{n, 1}; }

// get_points / get_points_keys: no downsample leaves more points than it was given
inline S3Bound s3_bound_get_points(const S3JobTable &tab) { return S3Bound{tab.total, (int64_t)tab.jobs.size()}; }

// compact_selected: a selection keeps at most every point of its cloud (handles are valid; a cloud named twice counts twice)
inline S3Bound s3_bound_compact(const Store3Slots &t, const int32_t *handles, int n_jobs)
{
    S3Bound b{0, n_jobs};
    for (int j = 0; j < n_jobs; ++j)
        b.points += t.cnt[(size_t)handles[j]];
    return b;
}
