// wgrt_seg.h -- the diagnostic segment stamps of a launch-tail pass (-DWGRT_SEG, tools/segments.py);
// every macro is empty in the product build.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace wgrt {

// Diagnostic segment stamps of a launch-tail pass (tools/segments.py).  Only a build with
// -DWGRT_SEG (an experimental library, never the product) executes any of this: s_memtime at fixed
// points of the pass, each segment's shader cycles summed per wave in scalar registers, and forced
// vmcnt(0) waits at the ends of the two load segments, which separate a load's wait from the arithmetic
// that overlaps it in the real kernel -- so the build's SHARES are read, not its length.
// s[0] advance, s[1] retire / ballots, s[2] line-0 loads + the draw and bound arithmetic until they have
// landed, s[3] estimate + decision, s[4] the taken branch's cell word, hop and matrix until landed,
// s[5] field update, s[6] the rest of the pass (in-coupler test, outcome, out-coupling queue), s[7] passes.
// The sums live in the wave's own LDS words (p[0..7], p[8] = the last stamp), updated by the wave's first
// active lane: a mark inside exec-masked code then still adds to the wave's sums (register sums there
// become per-lane vector values).  32-bit sums of 32-bit differences: a tail is < 2^32 cycles.
struct SegAcc {
    uint32_t __attribute__((address_space(3))) *p;
};
#ifdef WGRT_SEG
__device__ __forceinline__ uint32_t seg_stamp() {
    unsigned long long t;
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
    __builtin_amdgcn_sched_barrier(0);
    return (uint32_t)t;
}
#define SEG_WAITVM(sg)                                        \
    do {                                                      \
        if (sg) asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); \
    } while (0)
// dep: a value the segment computes; the stamp takes it as an operand, so the compiler cannot sink
// that arithmetic past the stamp (IR passes move arithmetic across an asm statement otherwise)
__device__ __forceinline__ uint32_t seg_stamp_dep(double dep) {
    unsigned long long t;
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t) : "v"(dep) : "memory");
    __builtin_amdgcn_sched_barrier(0);
    return (uint32_t)t;
}
__device__ __forceinline__ bool seg_first_lane() {
    return (threadIdx.x & 63) == __builtin_amdgcn_readfirstlane(threadIdx.x & 63);
}
#define SEG_MARK_DEP(sg, k, dep)                              \
    do {                                                      \
        if (sg) {                                             \
            const uint32_t t_ = seg_stamp_dep((double)(dep)); \
            if (seg_first_lane()) {                           \
                (sg)->p[k] += t_ - (sg)->p[8];                \
                (sg)->p[8] = t_;                              \
            }                                                 \
        }                                                     \
    } while (0)
#define SEG_MARK(sg, k) SEG_MARK_DEP(sg, k, 0.0)
#if WGRT_SEG == 2
// -DWGRT_SEG=2: wave-uniform marks only (the top level of a pass, jones_body); the interior marks below
// sit in exec-masked code, whose stamps run only when a lane is there and whose sums the compiler merges
// in vector registers
#define SEG_IWAITVM(sg) ((void)0)
#define SEG_IMARK_DEP(sg, k, dep) ((void)0)
#else
#define SEG_IWAITVM(sg) SEG_WAITVM(sg)
#define SEG_IMARK_DEP(sg, k, dep) SEG_MARK_DEP(sg, k, dep)
#endif
#else
#define SEG_IWAITVM(sg) ((void)0)
#define SEG_IMARK_DEP(sg, k, dep) ((void)0)
#define SEG_WAITVM(sg) ((void)0)
#define SEG_MARK(sg, k) ((void)0)
#define SEG_MARK_DEP(sg, k, dep) ((void)0)
#endif
// -DWGRT_SEG=2: wave-uniform segment marks at the top level of a pass (tools/segments.py)
#if defined(WGRT_SEG) && WGRT_SEG == 2
#define SEG_TMARK(sg, k, dep) SEG_MARK_DEP(sg, k, dep)
#else
#define SEG_TMARK(sg, k, dep) ((void)0)
#endif

}  // namespace wgrt
