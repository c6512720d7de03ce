// The proposals (GA && SH) family of rollout_persist_kernel, an object of its own: the horizon
// kernels of drpo_rollout_trajectories_proposed, under either shield. persist_run (rollout.hip)
// calls in here; in a -DDRPO_STAMPS build these kernels carry no stamps (rollout_persist.hpp).
#include "rollout_persist.hpp"

void launch_persist_proposed(int rpt, bool lw, bool paired, bool pg, const PersistArgs& a, size_t lds_bytes,
                             hipStream_t stream) {
  launch_persist_family<true, true>(rpt, lw, paired, pg, a, lds_bytes, stream);
}
