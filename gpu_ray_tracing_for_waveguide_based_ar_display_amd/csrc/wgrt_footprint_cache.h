// wgrt_footprint_cache.h -- the per-wave counter cache in front of an int64 footprint map, shared by the footprint
// launch's Jones-vector lane (wgrt_trace.hip, the FP instantiations) and the reduction of a path list
// (wgrt_paths.hip).
//
// One 8-byte atomic per count is one 64-B request at the memory side, and a kernel of them runs at the chip's atomic
// request rate whatever else it does (DESIGN.md §4.7 has the figures), so the counts are summed on chip first: every
// wave keeps a direct-mapped cache of kFpSlots counters in LDS, an entry (offset + 1) << 20 | count.  A count whose
// entry is cached is one LDS add; one whose slot holds another entry (or none) swaps its own entry in with count 1 and
// adds what it swapped out to the map with one global atomic; the wave adds what its cache still holds when it ends.
// (What it merges depends on the map: everything on a coarse one; at 256 x 256 cells a wave's counts rarely meet again,
// and the gain measured there is smaller: DESIGN.md §4.7.)  The cache is the wave's own -- no other wave touches it,
// and a wave's LDS operations execute in order -- so a lane's read, the matching lanes' adds and then the other lanes'
// swaps need no lock: whatever a swap takes out, adds included, goes to the map exactly once.  (A workgroup-wide cache
// would merge four times as many counts but needs a compare-and-swap loop per count, which the in-coupler's few cells
// would serialise.)
// Without the cache (wgrt_debug_set_footprint_aggregate(0)): one global atomic per count.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace wgrt {

constexpr int kFpSlots = 512;             // per wave: 4 KB of LDS
constexpr int kFpCountBits = 20;          // an entry's count stays below 2^20: a fuller one is swapped out
typedef unsigned long long __attribute__((address_space(3))) LdsU64;
static_assert((kFpSlots & (kFpSlots - 1)) == 0 && kFpSlots <= 65536, "fp_slot takes the product's top bits");
__device__ __forceinline__ int fp_slot(uint64_t key) {
    return (int)(((uint32_t)key ^ (uint32_t)(key >> 32)) * 2654435761u >> 16) & (kFpSlots - 1);
}
// One count at map offset off (< 0: none) through the wave's cache; called by every lane of the wave.
__device__ __forceinline__ void fp_cached(LdsU64 *tab, int64_t *map, int64_t off) {
    constexpr uint64_t kCountMask = (1ull << kFpCountBits) - 1ull;
    const bool todo = off >= 0;
    const uint64_t key = (uint64_t)off + 1ull;   // (never 0: an empty slot matches nothing)
    LdsU64 *const e = tab + fp_slot(key);
    bool hit = false;
    if (todo) {
        const uint64_t cur = *e;
        // (64 lanes may add to one entry in this pass: the count stays within its bits)
        hit = (cur >> kFpCountBits) == key && (cur & kCountMask) < kCountMask - 64ull;
    }
    if (hit) __hip_atomic_fetch_add(e, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    asm volatile("" ::: "memory");   // the adds are issued before the swaps
    if (todo && !hit) {
        const uint64_t old = __hip_atomic_exchange(e, (key << kFpCountBits) | 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (old != 0ull)
            atomicAdd((unsigned long long *)map + ((old >> kFpCountBits) - 1ull), (unsigned long long)(old & kCountMask));
    }
    asm volatile("" ::: "memory");
}
// What the wave's cache still holds, added to the map: one global atomic per entry.
__device__ __forceinline__ void fp_flush(LdsU64 *tab, int64_t *map) {
    constexpr uint64_t kCountMask = (1ull << kFpCountBits) - 1ull;
    asm volatile("" ::: "memory");
    for (int k = threadIdx.x & 63; k < kFpSlots; k += 64) {
        const uint64_t v = tab[k];
        if (v != 0ull) atomicAdd((unsigned long long *)map + ((v >> kFpCountBits) - 1ull), (unsigned long long)(v & kCountMask));
    }
}

}  // namespace wgrt
