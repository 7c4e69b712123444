// sa_band_nw_stats.hip -- banded NW statistics (seqalign_nw_stats_banded): for each pair the banded end value of
// seqalign_nw_score_banded and the matches and mismatches of the alignment inside the band that ends there, nothing stored per
// cell, no walk.  StatSweep's row arithmetic (sa_nw_stats.hpp; the definition of the payloads, the mark and the tie rule:
// sa_nw_stats.hip's header) inside the NW band frame, band_nw_payload_rows_kernel<BandNwStatsFrame, CPL, SUBST,
// GENERAL> (sa_band_nw_frame.hpp's header: the frame, the four rules of payloads in it, why no band cell reads a position
// outside the band).  DESIGN.md 3.25.
#include "sa_nw_stats.hpp"
#include "sa_band_nw_frame.hpp"

hipError_t sa_launch_band_nw_stats(const SaBandNwStatsParams &p, uint32_t max_width, hipStream_t stream) {
  return sa::launch_band_nw_payload<sa::BandNwStatsFrame>(p, max_width, stream);
}
