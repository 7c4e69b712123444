// sa_band_nw_gaps.hip -- banded NW gap-run counts at any band width (seqalign_nw_gaps_banded, seqalign_nw_gaps_banded_wide): for
// each pair the banded end value of seqalign_nw_score_banded[_wide] and the numbers of '-' runs in the two strings of the
// alignment inside the band that ends there (seqalign_nw_align_banded[_wide]'s), nothing stored per cell, no walk.  NwGapSweep's
// row arithmetic (sa_nw_gaps.hpp; the definition of the two words, the border's runs and the mark: sa_nw_gaps.hip's header,
// DESIGN.md 3.34) inside the NW band frame of sa_band_nw_frame.hpp, whose rules hold unchanged: the floor and the mark outside
// the band, the reset above the right edge, the three phases of the left feed.  Only the border's payloads differ from the
// statistics': row 0 is NwGapSweep::start_strip's (0, 1), the border column while it is in the band carries (1, 0) in both of
// its payloads, and a pair with len_a = 0 < len_b is one run of gap_a columns.  The sweep decides its increments from the row
// number (j = 1: the row above is the border) and from col0 = 0 (the cell left of column 1 is the border column's), both of
// which the frame hands it as the unbanded kernels do; a cell outside the band carries the mark, so what is added to it is
// never read.
//
// The narrow kernel is band_nw_payload_rows_kernel<BandNwGapsFrame, CPL, SUBST, GENERAL>: one wave per pair, 4 pairs per
// workgroup, CPL from {1 .. 6, 8} by the launch's widest band.  The wide kernel is band_nw_payload_strips_kernel<BandNwGapsFrame,
// ..>: one wave per (pair, strip of 64 | 128 | 256 | 512 columns).  Recorded as "band_score".
#include "sa_nw_gaps.hpp"
#include "sa_band_nw_frame.hpp"

namespace sa {

// the NW gap-run family of the band frame: word 0 gap_runs_a, word 1 gap_runs_b | mark
struct BandNwGapsFrame {
  using Params = SaBandNwGapsParams;
  template <int CPL, int SUBST, bool GENERAL>
  using Sweep = NwGapSweep<CPL, SUBST, GENERAL>;
  static constexpr uint32_t kBorderX = 1u;   // a cell (0, y), y > 0: one run of gap_a columns
};

}  // namespace sa

hipError_t sa_launch_band_nw_gaps(const SaBandNwGapsParams &p, uint32_t max_width, hipStream_t stream) {
  return sa::launch_band_nw_payload<sa::BandNwGapsFrame>(p, max_width, stream);
}
hipError_t sa_launch_band_nw_gaps_strips(const SaBandWideParams<SaBandNwGapsParams> &p, uint32_t strip_cols, uint64_t items, hipStream_t stream) {
  return sa::launch_band_nw_payload_strips<sa::BandNwGapsFrame>(p, strip_cols, items, stream);
}
