// Host-side bookkeeping of the 3-D keyframe store (sfe_store3.hip): the slot table and the pool's fill level.  Plain C++
// without a HIP call, so that tests/host/store3_slots_check.cpp can run it on the CPU under the sanitizers.
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
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

struct Store3Slots {
    int64_t capacity = 0;   // points
    int64_t top = 0;        // points in use = offset of the next cloud
    int32_t max_clouds = 0;
    int32_t n_slots = 0;    // slots in use = the next handle
    std::vector<int64_t> stamp, off, cnt;

    void init(int64_t capacity_points, int32_t max_clouds_)
    {
        capacity = capacity_points;
        max_clouds = max_clouds_;
        top = 0;
        n_slots = 0;
        stamp.assign((size_t)max_clouds_, 0);
        off.assign((size_t)max_clouds_, 0);
        cnt.assign((size_t)max_clouds_, 0);
    }

    // (written as differences: capacity - top and max_clouds - n_slots cannot overflow, a sum of the arguments could)
    bool fits(int64_t points, int64_t slots) const
    {
        return points >= 0 && slots >= 0 && points <= capacity - top && slots <= (int64_t)max_clouds - (int64_t)n_slots;
    }

    bool valid(int64_t handle) const { return handle >= 0 && handle < (int64_t)n_slots; }

    // -> the new handle, or -1 if the cloud does not fit (nothing changes then)
    int32_t push(int64_t stamp_, int64_t n)
    {
        if (!fits(n, 1))
            return -1;
        const int32_t h = n_slots;
        stamp[(size_t)h] = stamp_;
        off[(size_t)h] = top;
        cnt[(size_t)h] = n;
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
            top = off[(size_t)n]; // where the first released cloud began
            n_slots = (int32_t)n;
        }
        return true;
    }
};
