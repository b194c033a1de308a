// The sizing rules of the peak pass (mtm_k_peaks.hip.h), written once: the launchers of mtm_peaks.hip apply them - for the
// search calls and the test-support entry mtm_debug_peak_pass alike -, plan_call and fm_begin size the candidate hash
// table with them, and the host checks (tests/native/sanitize_host.cpp) walk every rule.  Plain C++: no HIP type, no context.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/mtm_hip.h"

namespace mtm {

// rows of a score map for the 3x3 scans (peaks_kernel, refine_scan_kernel): a wave owns kPkCols columns x kPkRows rows
// (the flagged-segment scan: kPkSparseRows rows), a work-group is 4 waves stacked vertically
constexpr int kPkCols = 256, kPkRows = 32;
constexpr int kPkSparseRows = 8;

// floats per score-map row on the device
inline int map_pitch_of(int ow) { return (ow + 3) / 4 * 4; }

// grid of the peak scans: strips of 4 * strip_rows rows x kPkCols columns over the largest 2-D map, one layer per map
struct PeakGrid {
    unsigned x, y, z;
};
inline PeakGrid peak_grid_dims(int max_oh, int max_ow, int n_maps, int strip_rows) {
    return PeakGrid{(unsigned)((max_ow + kPkCols - 1) / kPkCols), (unsigned)((max_oh + 4 * strip_rows - 1) / (4 * strip_rows)),
                    (unsigned)n_maps};
}

// records of one (map, strip column) list of the flagged-segment scan: an eighth of the hit capacity, all lists together
// at most 64 MB, never fewer than 256
inline unsigned long long peak_list_cap(unsigned long long hit_cap, unsigned long long n_lists) {
    const unsigned long long by_mem = (64ull << 20) / sizeof(mtm_hit) / n_lists;
    const unsigned long long c = hit_cap / 8 < by_mem ? hit_cap / 8 : by_mem;
    return c > 256ull ? c : 256ull;
}

// work-groups of 256 candidates of the two verifiers (one thread per candidate, no stride: the candidate list holds
// min(hit_cap, 4096 * 256) records)
inline unsigned verify_blocks(long long hit_cap) {
    const long long b = (hit_cap + 255) / 256;
    return (unsigned)(b < 4096 ? b : 4096);
}

// slots of the candidate hash table: the smallest power of two >= 1024 and >= 2 * cand_cap; its keys (8 bytes a slot,
// 0 = empty) are cleared before every insertion pass, the values (4 bytes a slot) follow them in memory
inline size_t cand_hash_slots(long long cand_cap) {
    size_t hsz = 1024;
    while (hsz < 2 * (size_t)cand_cap) hsz <<= 1;
    return hsz;
}
inline size_t cand_hash_key_bytes(unsigned mask) { return ((size_t)mask + 1) * sizeof(unsigned long long); }
inline size_t cand_hash_bytes(unsigned mask) { return ((size_t)mask + 1) * (sizeof(unsigned long long) + sizeof(int)); }

// work-groups per map of the extremum launches (256 threads each, grid-stride over the map's pixels)
inline int extremum_blocks() { return 256; }
inline int extremum_batch_blocks(long long max_px) {
    const long long b = (max_px + 4095) / 4096;
    return (int)(b < 256 ? b : 256);
}

}  // namespace mtm
