// The persistent streaming round (round_sweep.hip) at k = 1..7: 84 of k_round_sweep's 116 instantiations,
// in a translation unit of their own so that they compile beside the k = 8 kernels, not after them.
// Built with the same build knobs as round_sweep.hip (the Makefile's variant target compiles both).
#include "sweep_kernel.h"

namespace avk {

hipError_t launch_round_sweep_lowk(const RoundParams& p, int k, SweepMode mode, uint32_t blocks, hipStream_t s,
                                   bool* ref_written) {
  return dispatch_k<7>(k, [&](auto K) { return launch_sweep_k<K()>(p, mode, blocks, s, ref_written); });
}

hipError_t round_sweep_occupancy_lowk(int k, bool replay, int* blocks_per_cu) {
  return dispatch_k<7>(k, [&](auto K) { return occupancy_k<K()>(replay, blocks_per_cu); });
}

}  // namespace avk
