// sa_band_nw_stats_strips.hip -- wide banded NW statistics (seqalign_nw_stats_banded_wide): seqalign_nw_stats_banded's three
// integers at any band width, one pair on many waves.  StatSweep's row arithmetic (sa_nw_stats.hpp) in the wide NW band frame,
// band_nw_payload_strips_kernel<BandNwStatsFrame, CPL, SUBST, GENERAL> (sa_band_nw_frame.hpp's header: the strip pipeline, the
// payload rules per strip, the hand-off and the result).  DESIGN.md 3.26.
#include "sa_nw_stats.hpp"
#include "sa_band_nw_frame.hpp"

hipError_t sa_launch_band_nw_stats_strips(const SaBandWideParams<SaBandNwStatsParams> &p, uint32_t strip_cols, uint64_t items, hipStream_t stream) {
  return sa::launch_band_nw_payload_strips<sa::BandNwStatsFrame>(p, strip_cols, items, stream);
}
