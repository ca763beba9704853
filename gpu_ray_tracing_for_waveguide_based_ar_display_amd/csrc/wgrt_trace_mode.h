// wgrt_trace_mode.h -- the mode of a Jones-vector trace launch, stated once: the template axis of jones_body and of
// the mode kernels, the first index of the kernel table and of the scene's grid table, and LaunchCfg::mode
// (wgrt_trace.hip).  A launch has exactly one mode; what combines freely with it (fused, single wavelength, AMP, the
// locator's form, the cell width) stays an axis of its own.
#pragma once

namespace wgrt {

enum class TraceMode : int {
    kPlain,      // the product launches: every combination of the free axes is built
    kTimeline,   // the debug wave timeline (wgrt_debug_opts.timeline): 32-bit cells, full colour, no AMP; fused or not
    kLearn,      // a learning launch of the automatic issue order (wgrt_order.h): full colour, no AMP
    kChain,      // a step of a chain of single launches (wgrt_chain_*): full colour
    kFate,       // stores every ray's fate code (wgrt_trace_fate)
    kReps,       // fills replica window tables (wgrt_trace_replicas)
    kEv,         // the expected-value estimator (wgrt_trace_expected)
    kFp,         // counts every draw into the footprint maps (wgrt_trace_footprint)
    kHits,       // appends one record per out-coupling to the hit list (wgrt_trace_hits)
    kPaths,      // appends one record per draw of the selected rays to the path list (wgrt_trace_paths)
    kVisits,     // counts the taken branches of the counted rays per channel (wgrt_trace_visits)
    kStokes,     // adds every counted out-coupling's Stokes quanta to the tables beside the window table (wgrt_trace_stokes)
    kCount
};
constexpr int kTraceModes = (int)TraceMode::kCount;

}  // namespace wgrt
