// launch_grid.hpp -- how many workgroups a one-dimensional launch gets.  Plain C++ (no HIP include): a host compiler builds it,
// and tests/test_launch_grid.py holds its arithmetic to the limits below without a device.
//
// HIP refuses a launch whose gridDim.x * blockDim.x exceeds 2^32 - 1 (hipErrorInvalidConfiguration), so with 256-lane
// workgroups a grid has at most 16 777 215 of them.  Kernels with a grid-stride loop take grid_for(): one workgroup per `threads`
// work items up to that limit (or a cap of their own, measured), and the loop walks what lies beyond it.  Kernels whose grid IS
// their index space check launch_fits() and fall back or fail.
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstdlib>

namespace heamd {
namespace launch_grid {

constexpr size_t kMaxLanes = 0xffffffffu;  // gridDim.x * blockDim.x of one launch

// ceil(work_items / threads), at least 1 and at most cap (cap 0 counts as 1); no intermediate wraps for any size_t input
constexpr size_t grid_blocks(size_t work_items, unsigned threads, size_t cap) {
    const size_t t = threads ? threads : 1;
    const size_t blocks = work_items / t + (work_items % t != 0 ? 1 : 0);
    const size_t least = blocks ? blocks : 1;
    return least < cap ? least : (cap ? cap : 1);
}

constexpr size_t max_blocks(unsigned threads) { return kMaxLanes / (threads ? threads : 1); }

// a fixed grid of `blocks` workgroups of `threads` lanes can be launched
constexpr bool launch_fits(size_t blocks, unsigned threads) { return blocks <= max_blocks(threads); }

// HEAMD_GRID_CAP=<workgroups> lowers every strided launch's grid (the tests: a lane that makes several trips through its loop
// must give the words of one that makes a single trip).  Read at the call; unset, empty, zero or not a number: no override.
inline size_t grid_cap_override() {
    const char* forced = std::getenv("HEAMD_GRID_CAP");
    if (forced == nullptr || *forced == '\0') return SIZE_MAX;
    for (const char* c = forced; *c != '\0'; ++c)
        if (*c < '0' || *c > '9') return SIZE_MAX;
    const unsigned long long want = std::strtoull(forced, nullptr, 10);
    return want == 0 || want >= SIZE_MAX ? SIZE_MAX : static_cast<size_t>(want);  // (too many digits saturate: no override)
}

// Grid of a kernel that strides over `work_items`: one workgroup per `threads` items, never more than the kernel's own cap, than
// what HIP launches, or than the override -- the minimum of the three.
inline unsigned grid_for(size_t work_items, unsigned threads = 256, size_t own_cap = SIZE_MAX) {
    size_t cap = max_blocks(threads);
    if (own_cap < cap) cap = own_cap;
    const size_t forced = grid_cap_override();
    if (forced < cap) cap = forced;
    return static_cast<unsigned>(grid_blocks(work_items, threads, cap));
}

// The same for kernels in which a whole workgroup takes one item and strides by gridDim.x
inline unsigned grid_for_blocks(size_t block_items, unsigned threads, size_t own_cap = SIZE_MAX) {
    const size_t limit = max_blocks(threads);
    return grid_for(block_items, 1, own_cap < limit ? own_cap : limit);
}

// Grid of a kernel in which every lane takes exactly one item (no loop, so no cap and no override): a count that HIP cannot
// launch stays above the limit, and the launch reports hipErrorInvalidConfiguration instead of covering part of the items.
inline unsigned exact_grid(size_t work_items, unsigned threads = 256) {
    return static_cast<unsigned>(grid_blocks(work_items, threads, kMaxLanes));
}

}  // namespace launch_grid
}  // namespace heamd
