// The 64-bit keys the score kernels reduce a map to (win_merge_key, extremum_kernel: order(value) << 32 | ~row-major
// index, merged by atomicMax) read back, as inline functions for the host (decode_quality_key and decode_extremum_key,
// mtm_host.cpp; decode_block_keys, mtm_blocks.hip) and the device (track_record, mtm_track.hip; blocks_record_kernel and
// blocks_nbhd_kernel, mtm_k_blocks.hip.h): a single source for the order word's float32, the index and the record, so that
// the record a call decodes on the host is the record a kernel writes, bit for bit.  key_float_order forms the order word
// where host and device share the code that builds a key (mtm_blocks_second.h).
#pragma once
#include <cstdint>

#include "../../include/mtm_hip.h"
#include "mtm_templ_stats.h"       // MTM_HOST_DEVICE

namespace mtm {

// The float32 of a key's high word: the inverse of mf_float_order (mtm_device_util.hip.h), which stores -0 as +0.
MTM_HOST_DEVICE inline float key_order_float(uint32_t o) {
    const uint32_t b = (o & 0x80000000u) ? (o ^ 0x80000000u) : ~o;
    float v;
    __builtin_memcpy(&v, &b, 4);
    return v;
}

// The order word of a float32, key_order_float's inverse: mf_float_order's bits (-0 stored as +0), for code that forms a
// key on the host as well as on the device (mtm_blocks_second.h).  The score kernels keep calling mf_float_order.
MTM_HOST_DEVICE inline uint32_t key_float_order(float v) {
    if (v == 0.0f) v = 0.0f;     // -0 -> +0
    uint32_t b;
    __builtin_memcpy(&b, &v, 4);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// The row-major index in a key's low word (stored complemented: of equal values the first output wins the atomicMax).
MTM_HOST_DEVICE inline uint32_t key_index(unsigned long long key) { return 0xFFFFFFFFu - (uint32_t)(key & 0xFFFFFFFFull); }

// The record of index `idx` in a map ow outputs wide whose output (0, 0) is pixel (x0, y0).
MTM_HOST_DEVICE inline mtm_hit key_record(uint32_t idx, float score, int templ_idx, int y0, int x0, int ow, int w, int h) {
    mtm_hit r;
    r.templ_idx = templ_idx;
    r.x = x0 + (int)(idx % (uint32_t)ow);
    r.y = y0 + (int)(idx / (uint32_t)ow);
    r.w = w;
    r.h = h;
    r.score = score;
    return r;
}

// The record of a window kernel's key - over the quality: the score, or -score for the difference methods (mode_min) -
// for template `templ_idx` (a w x h box).  The score is (mode_min ? -q : q) + 0.0f: a quality of -0 gives +0.  key == 0
// (no output was scored): the quiet NaN, at the index the key reads.
MTM_HOST_DEVICE inline mtm_hit quality_key_record(unsigned long long key, int mode_min, int templ_idx, int y0, int x0, int ow,
                                                  int w, int h) {
    const float q = key_order_float((uint32_t)(key >> 32));
    return key_record(key_index(key), key ? (mode_min ? -q : q) + 0.0f : __builtin_nanf(""), templ_idx, y0, x0, ow, w, h);
}

}  // namespace mtm
