// libmtm_hip.so - block matching between two images of one shape in one call (mtm_match_blocks): every block
// of the reference image is a template, searched in the other image inside the block's own box widened by a margin - what
// mtm_find_matches_boxes returns in MTM_PEAKS_GLOBAL mode for the block's pixels set as a template.  Both images go up as
// one stack of two (the reference in rows 0 .., the image below it); the kernels are mtm_k_blocks.hip.h's (and
// mtm_k_deform.hip.h's), this file is the host side: plan_blocks (mtm_host.cpp) checks the blocks and lays out the unit
// and tile tables and the chunks; the host waits once per call.  uint8 (1 or 3 channels) and single-channel uint16.  The
// template set of the context is neither read nor written.
// mtm_match_blocks_stack runs the same chain for every pair of a frame stack, which goes up in stacked
// chunks (plan_blocks_stack, mtm_host.cpp); every pair has a row of keys of its own, or - ensemble planes - a plane of sums.
// mtm_match_blocks_at / _second and the five mtm_match_blocks_passes* entries search boxes that
// follow a displacement - uploaded offsets, or the previous pass's records.  Each entry fills one record of what is asked
// for and where results go (BlockPassCall: validation, second peaks, deformation, steering; an absent feature is an empty
// field) behind one of two preambles (block_passes_entry, block_single_entry), and one chain runs it (match_block_passes):
// stage_block_passes (the passes' tables concatenated, second-peak sub-ranges, deform tables, stage_block_call), then per
// pass block_pass_view (the pass's device pointers and what it does, derived once), pass_search (the units it searches,
// or the warped image), blocks_pair, pass_records (record, deform-record, second-record, validate) and pass_handover
// (steer-q8, smooth), in stream order; every pass has its own row of keys, records and neighbourhoods.
// mtm_match_blocks_masked is the single-pass chain with a static mask over the reference: the mask goes up
// once into blk_mask behind the images, and every launch of blocks_pair is the masked sibling of the unmasked kernel.
// mtm_match_blocks_stack_at / mtm_match_blocks_stack_passes run the pass chain for the pairs of a frame stack
// (match_block_stack_passes): the same tables, views and launches, every pair with a row of keys, records and
// neighbourhoods of its own - or, ensemble planes, pass after pass over all pairs, the planes' peaks steering the next.
// Every entry point composes the same host steps: check_block_entry / check_block_pair, stage_block_call (buffers, the
// call's clock, uploads), blocks_pair (a pair's launch chain, the one place its kernels are launched), launch_lanes (the
// one-lane-per-block launches), finish_block_call (copies back, the single wait, timing); debug entries: debug_block_run.
#include <climits>
#include <type_traits>

#include "mtm_k_blocks.hip.h"

using namespace mtm;
using namespace mtmi;

namespace {

// f(ch, u16) with the images' pixel kind as compile-time constants, the kernels' <CH, U16>.
template <class F>
int blocks_dispatch(int dtype, int chans, F&& f) {
    if (dtype == MTM_U16) return f(std::integral_constant<int, 1>{}, std::true_type{});
    if (chans == 1) return f(std::integral_constant<int, 1>{}, std::false_type{});
    return f(std::integral_constant<int, 3>{}, std::false_type{});
}

// The one-lane-per-block launch: `kernel` over n lanes in work-groups of 256 on the call's stream.
template <class... P, class... A>
int launch_lanes(mtm_ctx* c, void (*kernel)(P...), size_t n, A&&... args) {
    hipLaunchKernelGGL(kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, static_cast<P>(args)...);
    HIPC(hipGetLastError());
    return MTM_OK;
}

// The image of rows row_off .. row_off + rows - 1 of the stack `st`: its planes entered at that row and bounded by `rows`,
// so that pixels below it read as zero whatever the stack holds there.
ImageDev stack_view(const ImageDev& st, int row_off, int rows) {
    ImageDev v = st;
    v.u8 = st.u8 + (size_t)row_off * st.u8_pitch;
    v.f32 = nullptr;
    v.rows = rows;
    return v;
}

// What both entry points check of their images behind check_image_args: the pixel kind, and that a pair's two images -
// one stack - stay within the rows a layout launch's grid holds.  `noun`: "images" / "frames", as the entry names them.
int check_block_images(const char* who, const std::string& noun, int rows, int chans, int dtype) {
    if (!((dtype == MTM_U8 && (chans == 1 || chans == 3)) || (dtype == MTM_U16 && chans == 1))) {
        set_error(std::string(who) + ": takes uint8 " + noun + " with 1 or 3 channels and single-channel uint16 " + noun);
        return MTM_E_INVALID;
    }
    if (2ll * rows > kBatchMaxRows) {
        set_error(std::string(who) + ": " + noun + " of more than " + std::to_string(kBatchMaxRows / 2) + " rows");
        return MTM_E_INVALID;
    }
    return MTM_OK;
}

// The host tables of a call, n blocks and n_tiles tiles in all (a multipass call: those of every pass, concatenated), and
// what the call needs besides them: `cells` float64 sums with the clip table (ensemble planes: cells > 0), or `key_rows`
// rows of n keys - with as many rows of neighbourhoods (nbhd), the uploaded offsets (offsets != nullptr), a row of records
// (recs) and of validation flags and steering records (validate); the second-peak calls: the plane offsets `poff` with
// plane_floats floats of planes (the largest launch sub-range's), a row of second keys and of their records.
struct BlockStage {
    const mtm_block* blocks;
    const long long* toff;
    const TrackUnit* units;
    const TrackTile* tiles;
    size_t n, n_tiles, max_bytes;
    size_t key_rows = 1, cells = 0;
    const int32_t *clip = nullptr, *offsets = nullptr;
    bool nbhd = false, recs = false, validate = false;
    const long long* poff = nullptr;
    size_t plane_floats = 0;
    // a deformed call: the weight tables of its deformed passes (dtab_words words), the warped image's bytes, the largest
    // steering grid's blocks and a row of Q8 fields at the blocks' centres
    const uint32_t* dtab = nullptr;
    size_t dtab_words = 0, warp_bytes = 0, disp_blocks = 0;
    bool deform = false;
    // ... steered by refined positions: the largest steering grid's unfiltered Q8 displacements
    size_t d8_blocks = 0;
};
BlockStage plan_stage(const mtm_block* blocks, const BlockPlan& P) {
    return BlockStage{blocks, P.toff.data(), P.units.data(), P.tiles.data(), P.units.size(), P.tiles.size(), P.max_bytes};
}

// The staging of every block call: the call's buffers, sized by S, then before() - what the entry enqueues ahead of the
// call's clock -, the event the call's time counts from, and the tables and zeroed results on the stream.
template <class Before>
int stage_block_call(mtm_ctx* c, const BlockStage& S, Before&& before) {
    const size_t n = S.n, n_keys = S.cells ? 0 : S.key_rows * n;
    // what goes up, in stream order (no source: not part of this call), and what is only sized
    const struct { DevBuf& buf; const void* src; size_t bytes; } up[] = {
        {c->blk_blocks, S.blocks, sizeof(mtm_block) * n},   {c->blk_toff, S.toff, sizeof(long long) * n},
        {c->blk_units, S.units, sizeof(TrackUnit) * n},     {c->blk_tiles, S.tiles, sizeof(TrackTile) * S.n_tiles},
        {c->blk_clip, S.clip, sizeof(int32_t) * 2 * n},     {c->blk_offs, S.offsets, sizeof(int32_t) * 2 * n},
        {c->blk_poff, S.poff, sizeof(long long) * n},       {c->blk_dtab, S.dtab, sizeof(uint32_t) * S.dtab_words}};
    const struct { DevBuf& buf; size_t bytes; } sized[] = {
        {c->blk_tpx, S.max_bytes},                          {c->blk_td, sizeof(TemplDev) * n},
        {c->blk_acc, sizeof(double) * S.cells},             {c->blk_keys, sizeof(unsigned long long) * n_keys},
        {c->blk_recs, S.recs ? sizeof(mtm_hit) * (S.cells ? n : S.key_rows * n) : 0},    {c->blk_nbhd, S.nbhd ? sizeof(float) * 9 * n_keys : 0},
        {c->blk_valid, S.validate ? n : 0},                 {c->blk_steer, S.validate ? sizeof(mtm_hit) * n : 0},
        {c->blk_plane, sizeof(float) * S.plane_floats},     {c->blk_keys2, S.poff ? sizeof(unsigned long long) * n : 0},
        {c->blk_recs2, S.poff ? sizeof(mtm_hit) * n : 0},   {c->blk_warp, S.warp_bytes},
        {c->blk_disp, sizeof(int32_t) * 2 * S.disp_blocks}, {c->blk_pred, S.deform ? sizeof(int32_t) * 2 * n : 0},
        {c->blk_d8, sizeof(int32_t) * 2 * S.d8_blocks}};
    HIPC(hipSetDevice(c->device));
    c->timing = mtm_timing{};
    c->maps_valid = false;
    c->last_hits.clear();
    for (const auto& u : up)
        if (u.src) MTMC(u.buf.ensure(u.bytes));
    for (const auto& s : sized) MTMC(s.buf.ensure(s.bytes));
    MTMC(before());
    HIPC(hipEventRecord(c->ev[0], c->stream));
    for (const auto& u : up)
        if (u.src) HIPC(hipMemcpyAsync(u.buf.p, u.src, u.bytes, hipMemcpyHostToDevice, c->stream));
    if (S.cells) HIPC(hipMemsetAsync(c->blk_acc.p, 0, sizeof(double) * S.cells, c->stream));
    else HIPC(hipMemsetAsync(c->blk_keys.p, 0, sizeof(unsigned long long) * n_keys, c->stream));
    if (S.deform) HIPC(hipMemsetAsync(c->blk_pred.p, 0, sizeof(int32_t) * 2 * n, c->stream));    // (pass 0 predicts nothing)
    return MTM_OK;
}

// The end of every block call's chain: the event its time counts to, the copies back (`dst` == nullptr: not asked for),
// the call's single wait and its timing; the stacks a call uploads are none of the caller's images (no current image).
struct BlockCopy {
    void* dst;
    const void* src;
    size_t bytes;
};
int finish_block_call(mtm_ctx* c, std::initializer_list<BlockCopy> copies, size_t n_hits) {
    HIPC(hipEventRecord(c->ev[1], c->stream));
    for (const BlockCopy& b : copies)
        if (b.dst) HIPC(hipMemcpyAsync(b.dst, b.src, b.bytes, hipMemcpyDeviceToHost, c->stream));
    HIPC(hipStreamSynchronize(c->stream));
    HIPC(hipEventElapsedTime(&c->timing.total_ms, c->ev[0], c->ev[1]));
    c->timing.n_hits = (int64_t)n_hits;
    c->have_image = false;
    return MTM_OK;
}

// The two images of a pair entry point, of one shape and pixel kind.
struct BlockPair {
    const void* reference;
    int64_t reference_stride_bytes;
    const void* image;
    int64_t image_stride_bytes;
    int rows, cols, chans, dtype;
};

// ONE upload of each image of a pair, ahead of the call's clock: the stack's rows 0 .. rows - 1 are the reference, rows ..
// 2 rows - 1 the image.
int upload_block_pair(mtm_ctx* c, const BlockPair& I) {
    adopt_image(c, 2 * I.rows, I.cols, I.chans, I.dtype);
    return upload_image_pair(c, c->slot[c->cur], I.reference, I.reference_stride_bytes, I.image, I.image_stride_bytes, I.rows,
                             I.cols, I.chans, I.dtype, c->stream);
}

// The preamble of every entry point with a chain: the context, the entry's own argument test (`args_ok`) and the method, as
// one "bad arguments"; then no call in flight.
int check_block_entry(mtm_ctx* c, const char* who, bool args_ok, int method) {
    if (!c || !args_ok || method < MTM_TM_SQDIFF || method > MTM_TM_CCOEFF_NORMED) {
        set_error(std::string(who) + ": bad arguments");
        return MTM_E_INVALID;
    }
    MTM_NOT_IN_FLIGHT(c, who);
    return MTM_OK;
}
// ... and of the pair entry points: both images, then what blocks ask of them.
int check_block_pair(mtm_ctx* c, const char* who, bool args_ok, int method, const BlockPair& I) {
    MTMC(check_block_entry(c, who, args_ok, method));
    MTMC(check_image_args(I.reference, I.rows, I.cols, I.chans, I.dtype, I.reference_stride_bytes, who));
    MTMC(check_image_args(I.image, I.rows, I.cols, I.chans, I.dtype, I.image_stride_bytes, who));
    return check_block_images(who, "images", I.rows, I.chans, I.dtype);
}

// What a pair's chain writes: a row of keys (and of neighbourhoods, or nullptr), or - side > 0, ensemble planes - the
// call's planes of sums, which the call's first pair starts.
struct BlockSink {
    unsigned long long* keys;
    float* nbhd;
    int side, first;
    // planes over the fixed tile table (units a kernel computed): the pass's planes of sums and its clip offsets, device
    double* acc = nullptr;
    const int32_t* clip = nullptr;
};

// The device tables a chain reads, indexed as its plan indexes them: the call's buffers from their start, or - one pass
// of several - from the pass's first block b0 and tile t0 (the constants td are every pass's in turn).  fixed: `tiles` is
// the fixed table (fix_block_tiles) and the units are the device's - blocks_score_fixed_kernel scores.
struct BlockTables {
    const mtm_block* blocks;
    const long long* toff;
    TemplDev* td;
    TrackUnit* units;
    const TrackTile* tiles;
    bool fixed;
};
BlockTables ctx_block_tables(mtm_ctx* c, size_t b0 = 0, size_t t0 = 0, bool fixed = false) {
    return BlockTables{c->blk_blocks.as<mtm_block>() + b0, c->blk_toff.as<long long>() + b0, c->blk_td.as<TemplDev>(),
                       c->blk_units.as<TrackUnit>() + b0, c->blk_tiles.as<TrackTile>() + t0, fixed};
}

// The floats block b's scored plane holds: the largest map a moved block can have, min(2 margin + 1, rows - h + 1) x
// min(2 margin + 1, cols - w + 1) (fix_block_tiles' spans: < 2^32) - known to the host whatever unit the device computes.
size_t second_plane_floats(const mtm_block& b, int margin, int rows, int cols) {
    const long long side = 2ll * margin + 1;
    return (size_t)std::min(side, (long long)rows - b.h + 1) * (size_t)std::min(side, (long long)cols - b.w + 1);
}

// What a second-peak pass adds to its chain (blocks_pair): the plan's blocks in sub-ranges of whole blocks - within a
// template-byte chunk, and their planes within `budget` floats, never fewer than one block -, each scored into the plane
// buffer (block k's plane at poff[k] floats) and reduced to keys2 by blocks_second_kernel before the next one overwrites it.
struct BlockSecondPass {
    int exclusion;
    std::vector<std::pair<int, int>> ranges;    // [b0, b1), in order, covering the pass
    std::vector<size_t> tstart;                 // block k's tiles are tiles[tstart[k] .. tstart[k + 1] - 1] of the pass
    const long long* poff;                      // device, indexed as the pass's tables
    unsigned long long* keys2;
};

// The sub-ranges and tile starts of plan P (fixed tile table) over `blocks`, the plane offsets appended to `poff` (one per
// block, relative to its sub-range's start) and the largest sub-range's floats raised into *max_floats.
void plan_second_pass(const BlockPlan& P, const mtm_block* blocks, int margin, int rows, int cols, size_t budget,
                      BlockSecondPass& X, std::vector<long long>& poff, size_t* max_floats) {
    const size_t n = P.units.size();
    X.tstart.assign(n + 1, P.tiles.size());
    for (size_t t = P.tiles.size(); t-- > 0;) X.tstart[(size_t)P.tiles[t].u0] = t;
    for (const BlockChunk& C : P.chunks) {
        int r0 = C.b0;
        size_t used = 0;
        for (int k = C.b0; k < C.b1; ++k) {
            const size_t f = second_plane_floats(blocks[k], margin, rows, cols);
            if (k > r0 && used + f > budget) {
                X.ranges.emplace_back(r0, k);
                r0 = k;
                used = 0;
            }
            poff.push_back((long long)used);
            used += f;
            *max_floats = std::max(*max_floats, used);
        }
        X.ranges.emplace_back(r0, C.b1);
    }
}

// One pair's launch chain for every block chunk - gather (unless the templates are already there), score or plane,
// [neighbourhoods] - in stream order: the next chunk's gather overwrites the template planes behind this chunk's last
// reader, and the host waits for none of them.  The pair is the stack's current image: the reference its rows
// r_slot * rows .., the searched image its rows i_slot * rows ...  X != nullptr (a second-peak pass over the fixed table):
// the chunk's score launch runs sub-range by sub-range with the scored-plane sink, blocks_second_kernel behind each.
// W != nullptr (a deformed pass): the searched image is *W with its low-byte plane W_lo - the warped image in a buffer
// of its own - instead of the stack's slot i_slot.
// mask != nullptr (mtm_match_blocks_masked: uint8 images, keys only): the call's mask plane on the device, `cols` bytes
// per row; every launch of the chain is then the masked sibling of the kernel named above, at the same place.
int blocks_pair(mtm_ctx* c, const BlockPlan& P, const BlockTables& B, int rows, int chans, int dtype, int method, int r_slot,
                int i_slot, bool gather, const BlockSink& S, const BlockSecondPass* X = nullptr, const ImageDev* W = nullptr,
                const uint8_t* W_lo = nullptr, const uint8_t* mask = nullptr) {
    const ImageDev st = image_dev(c);
    const uint8_t* st_lo = c->slot[c->cur].u8b.as<uint8_t>() + st.u8_plane;        // uint16: [high ^ 0x80][low ^ 0x80]
    const ImageDev ref = stack_view(st, r_slot * rows, rows), img = W ? *W : stack_view(st, i_slot * rows, rows);
    const uint8_t* ref_lo = st_lo + (size_t)r_slot * rows * st.u8_pitch;
    const uint8_t* img_lo = W ? W_lo : st_lo + (size_t)i_slot * rows * st.u8_pitch;
    const int mode_min = method_mode_min(method) ? 1 : 0;
    uint8_t* tpx = c->blk_tpx.as<uint8_t>();
    const long long* toff = B.toff;
    TemplDev* td = B.td;
    const TrackUnit* units = B.units;
    return blocks_dispatch(dtype, chans, [&](auto ch, auto u16) -> int {
        constexpr int CH = decltype(ch)::value;
        constexpr bool U16 = decltype(u16)::value;
        size_t xr = 0;          // (the second-peak sub-ranges are walked in step with the chunks)
        for (const BlockChunk& C : P.chunks) {
            if (gather)
                MTMC(for_launch_slices((size_t)C.b0, (size_t)C.b1, [&](size_t b0, unsigned nb) -> int {
                    if constexpr (!U16)
                        if (mask) {
                            hipLaunchKernelGGL((blocks_gather_masked_kernel<CH>), dim3(nb), dim3(256), 0, c->stream, ref, mask,
                                               ref.cols, B.blocks, (int)b0, tpx, toff, td, method);
                            HIPC(hipGetLastError());
                            return MTM_OK;
                        }
                    hipLaunchKernelGGL((blocks_gather_kernel<CH, U16>), dim3(nb), dim3(256), 0, c->stream, ref, ref_lo,
                                       B.blocks, (int)b0, tpx, toff, td, method);
                    HIPC(hipGetLastError());
                    return MTM_OK;
                }));
            for (; X && xr < X->ranges.size() && X->ranges[xr].second <= C.b1; ++xr) {
                const size_t r0 = (size_t)X->ranges[xr].first, r1 = (size_t)X->ranges[xr].second;
                MTMC(for_launch_slices(X->tstart[r0], X->tstart[r1], [&](size_t t0, unsigned nt) -> int {
                    if constexpr (!U16)
                        if (mask) {
                            hipLaunchKernelGGL((blocks_score_plane_masked_kernel<CH>), dim3(nt), dim3(256), 0, c->stream, img, tpx,
                                               toff, td, units, B.tiles + t0, method, mode_min, S.keys, c->blk_plane.as<float>(),
                                               X->poff);
                            HIPC(hipGetLastError());
                            return MTM_OK;
                        }
                    hipLaunchKernelGGL((blocks_score_plane_kernel<CH, U16>), dim3(nt), dim3(256), 0, c->stream, img, img_lo, tpx,
                                       toff, td, units, B.tiles + t0, method, mode_min, S.keys, c->blk_plane.as<float>(), X->poff);
                    HIPC(hipGetLastError());
                    return MTM_OK;
                }));
                MTMC(for_launch_slices(r0, r1, [&](size_t b0, unsigned nb) -> int {
                    hipLaunchKernelGGL(blocks_second_kernel, dim3(nb), dim3(256), 0, c->stream, units, S.keys,
                                       c->blk_plane.as<float>(), X->poff, (int)b0, mode_min, X->exclusion, X->keys2);
                    HIPC(hipGetLastError());
                    return MTM_OK;
                }));
            }
            if (!X) MTMC(for_launch_slices(C.t0, C.t1, [&](size_t t0, unsigned nt) -> int {
                if constexpr (!U16)
                    if (mask) {
                        if (B.fixed)
                            hipLaunchKernelGGL((blocks_score_masked_kernel<CH, true>), dim3(nt), dim3(256), 0, c->stream, img, tpx,
                                               toff, td, units, B.tiles + t0, method, mode_min, S.keys);
                        else
                            hipLaunchKernelGGL((blocks_score_masked_kernel<CH, false>), dim3(nt), dim3(256), 0, c->stream, img, tpx,
                                               toff, td, units, B.tiles + t0, method, mode_min, S.keys);
                        HIPC(hipGetLastError());
                        return MTM_OK;
                    }
                if (S.side > 0 && B.fixed)
                    hipLaunchKernelGGL((blocks_plane_fixed_kernel<CH, U16>), dim3(nt), dim3(256), 0, c->stream, img, img_lo, tpx,
                                       toff, td, units, B.tiles + t0, method, S.clip, S.side, S.first, S.acc);
                else if (S.side > 0)
                    hipLaunchKernelGGL((blocks_plane_kernel<CH, U16>), dim3(nt), dim3(256), 0, c->stream, img, img_lo, tpx, toff,
                                       td, units, B.tiles + t0, method, c->blk_clip.as<int32_t>(), S.side, S.first,
                                       c->blk_acc.as<double>());
                else if (B.fixed)
                    hipLaunchKernelGGL((blocks_score_fixed_kernel<CH, U16>), dim3(nt), dim3(256), 0, c->stream, img, img_lo, tpx,
                                       toff, td, units, B.tiles + t0, method, mode_min, S.keys);
                else
                    hipLaunchKernelGGL((blocks_score_kernel<CH, U16>), dim3(nt), dim3(256), 0, c->stream, img, img_lo, tpx, toff,
                                       td, units, B.tiles + t0, method, mode_min, S.keys);
                HIPC(hipGetLastError());
                return MTM_OK;
            }));
            if (S.nbhd)
                MTMC(for_launch_slices((size_t)C.b0, (size_t)C.b1, [&](size_t b0, unsigned nb) -> int {
                    if constexpr (!U16)
                        if (mask) {
                            hipLaunchKernelGGL((blocks_nbhd_masked_kernel<CH>), dim3(nb), dim3(256), 0, c->stream, img, tpx, toff,
                                               td, units, S.keys, (int)b0, method, S.nbhd);
                            HIPC(hipGetLastError());
                            return MTM_OK;
                        }
                    hipLaunchKernelGGL((blocks_nbhd_kernel<CH, U16>), dim3(nb), dim3(256), 0, c->stream, img, img_lo, tpx, toff,
                                       td, units, S.keys, (int)b0, method, S.nbhd);
                    HIPC(hipGetLastError());
                    return MTM_OK;
                }));
        }
        return MTM_OK;
    });
}

// A pair's row of keys as hits: each block's extremum in its own map, at the map's origin in image coordinates
// (quality_key_record: blocks_record_kernel's function).
void decode_block_keys(const BlockPlan& P, const mtm_block* blocks, const unsigned long long* hkeys, int method, mtm_hit* out) {
    const int mode_min = method_mode_min(method) ? 1 : 0;
    for (size_t k = 0; k < P.units.size(); ++k) {
        const TrackUnit& u = P.units[k];
        out[k] = quality_key_record(hkeys[k], mode_min, (int)k, u.y0, u.x0, u.ow, blocks[k].w, blocks[k].h);
    }
}

// The weight tables of the warp by the field of grid g over a rows x cols image, appended to t: deform_pack_inl of
// deform_axis_inl per column (padded with the last column's word to a multiple of kDeformPx) and per row (padded
// likewise, so that the next tables start 32-byte aligned).  Returns the column table's first word.
size_t deform_tables(const BlockGrid& g, int rows, int cols, std::vector<uint32_t>& t) {
    const size_t at = t.size();
    auto axis = [&](int n, int s, int wc, int len) {
        uint32_t w = 0;
        for (int x = 0; x < len; ++x) {
            int i, a8;
            deform_axis_inl(n, s, wc, 2ll * x, &i, &a8);
            t.push_back(w = deform_pack_inl(i, a8));
        }
        while (t.size() % kDeformPx) t.push_back(w);
    };
    axis(g.nx, g.sx, g.bw, cols);
    axis(g.ny, g.sy, g.bh, rows);
    return at;
}
size_t deform_table_rows_at(int cols) { return (size_t)(cols + kDeformPx - 1) / kDeformPx * kDeformPx; }

// The warped image of a call: byte planes of `pitch` bytes per row in blk_warp, `rows` rows each.
size_t warp_bytes(int rows, int pitch, int chans, int dtype) { return (size_t)rows * pitch * (dtype == MTM_U16 ? 2 : chans); }
ImageDev warp_view(const mtm_ctx* c, int rows, int cols, int chans) {
    ImageDev v{};
    v.u8 = c->blk_warp.as<uint8_t>();
    v.rows = rows;
    v.cols = cols;
    v.chans = chans;
    v.u8_pitch = c->u8_pitch;
    v.u8_plane = (long long)c->u8_pitch * rows;
    return v;
}

// The warp launch: `src` (its low-byte plane src_lo) warped into the call's blk_warp by the field of grid g with the
// displacements in blk_disp - q8: Q8 nodes - and the tables at word `tab` of blk_dtab.
int launch_deform(mtm_ctx* c, const ImageDev& src, const uint8_t* src_lo, int chans, int dtype, const BlockGrid& g, size_t tab,
                  bool q8 = false) {
    const ImageDev dst = warp_view(c, src.rows, src.cols, chans);
    DeformArgs a{};
    a.src = src.u8;
    a.src_lo = src_lo;
    a.src_plane = src.u8_plane;
    a.src_pitch = src.u8_pitch;
    a.dst = c->blk_warp.as<uint8_t>();
    a.dst_lo = a.dst + dst.u8_plane;
    a.dst_plane = dst.u8_plane;
    a.dst_pitch = dst.u8_pitch;
    a.rows = src.rows;
    a.cols = src.cols;
    a.disp = c->blk_disp.as<int32_t>();
    a.nx = g.nx;
    a.ny = g.ny;
    a.colw = c->blk_dtab.as<uint32_t>() + tab;
    a.roww = a.colw + deform_table_rows_at(src.cols);
    const dim3 grd((unsigned)((src.cols + kDeformLanesX * kDeformPx - 1) / (kDeformLanesX * kDeformPx)),
                   (unsigned)((src.rows + 256 / kDeformLanesX - 1) / (256 / kDeformLanesX)));
    return blocks_dispatch(dtype, chans, [&](auto ch, auto u16) -> int {
        if (q8)
            hipLaunchKernelGGL((deform_image_kernel<decltype(ch)::value, decltype(u16)::value, true>), grd, dim3(256), 0, c->stream,
                               a);
        else
            hipLaunchKernelGGL((deform_image_kernel<decltype(ch)::value, decltype(u16)::value>), grd, dim3(256), 0, c->stream, a);
        HIPC(hipGetLastError());
        return MTM_OK;
    });
}

// What a call of the pass chain asks for and where its results go (host memory, pass-major); an absent feature is an
// empty field, and a chain without it launches and copies exactly what it would if the feature did not exist.
struct BlockPassCall {
    int method;
    mtm_hit* out;                       // every pass's records
    float* nbhd;                        // ... and their neighbourhoods (nullptr: not asked for)
    const int32_t* offsets = nullptr;   // mtm_match_blocks_at / _second: pass 0 follows an uploaded displacement per block
    uint8_t* valid = nullptr;           // validation: the median test behind every pass's records - its flags,
    double threshold = 0.0, epsilon = 0.0;      // threshold and epsilon -, which steer the next pass instead of the raw ones
    mtm_hit* second = nullptr;          // second peaks: every pass's second records, which steer nothing;
    int exclusion = 0;                  //   the exclusion radius around the first peak
    int32_t* predicted = nullptr;       // deformation (never with offsets or second): the Q8 field at every block's centre;
    int steer = 0;                      //   0 - integer records steer the next pass -, 1 - refined positions, filtered
    const void* mask = nullptr;         // mtm_match_blocks_masked (one pass, uint8): the mask over the reference, rows x cols
    int64_t mask_stride_bytes = 0;      //   bytes, non-zero = the pixel takes part; never with deformation or validation
    bool plan_tiles = false;            //   the pass scores over the plan's own tile table (no offsets, no second peaks)
};

// What stage_block_passes lays out on the host for the whole call: the tables of every pass, concatenated (one upload
// each); second peaks: every pass's plane sub-ranges and one table of plane offsets; deformation: the weight tables of
// every pass p >= 1 (those of pass p - 1's grid), pass p's at word dtab_at[p].
struct BlockPassHost {
    std::vector<mtm_block> blocks;
    std::vector<long long> toff, poff;
    std::vector<TrackUnit> units;
    std::vector<TrackTile> tiles;
    std::vector<BlockSecondPass> X;
    std::vector<uint32_t> dtab;
    std::vector<size_t> dtab_at;
};

// Stage the call: H and what the buffers they and the asked-for results need (pass_stage: the host side, shared with the
// stack form), both images up once, then the call's clock and the tables (stage_block_call).  steer = 1 with a pass to
// steer: the neighbourhoods exist whether or not the caller asked.
BlockStage pass_stage(mtm_ctx* c, const BlockPair& I, const std::vector<BlockPassPlan>& Q, const BlockPassCall& A,
                      BlockPassHost& H) {
    size_t max_bytes = 0;
    for (const BlockPassPlan& q : Q) {
        H.blocks.insert(H.blocks.end(), q.blocks.begin(), q.blocks.end());
        H.toff.insert(H.toff.end(), q.plan.toff.begin(), q.plan.toff.end());
        H.units.insert(H.units.end(), q.plan.units.begin(), q.plan.units.end());
        H.tiles.insert(H.tiles.end(), q.plan.tiles.begin(), q.plan.tiles.end());
        max_bytes = std::max(max_bytes, q.plan.max_bytes);
    }
    BlockStage S{H.blocks.data(), H.toff.data(), H.units.data(), H.tiles.data(), H.blocks.size(), H.tiles.size(), max_bytes};
    S.nbhd = A.nbhd != nullptr, S.offsets = A.offsets;
    S.recs = true, S.validate = A.valid != nullptr;
    if (A.second) {
        H.X.resize(Q.size());
        H.poff.reserve(S.n);
        for (size_t p = 0; p < Q.size(); ++p) {
            H.X[p].exclusion = A.exclusion;
            plan_second_pass(Q[p].plan, Q[p].blocks.data(), Q[p].margin, I.rows, I.cols, (size_t)c->boxes_max_floats, H.X[p],
                             H.poff, &S.plane_floats);
        }
        S.poff = H.poff.data();
    }
    H.dtab_at.assign(Q.size(), 0);
    if (A.predicted) {
        for (size_t p = 1; p < Q.size(); ++p) {
            H.dtab_at[p] = deform_tables(Q[p - 1].grid, I.rows, I.cols, H.dtab);
            S.disp_blocks = std::max(S.disp_blocks, Q[p - 1].blocks.size());
        }
        S.deform = true;
        if (A.steer && Q.size() > 1) {
            S.d8_blocks = S.disp_blocks;
            S.nbhd = true;
        }
        S.dtab = H.dtab.empty() ? nullptr : H.dtab.data(), S.dtab_words = H.dtab.size();
        if (Q.size() > 1) S.warp_bytes = warp_bytes(I.rows, (int)round_up((size_t)I.cols + kPadCols, 64), I.chans, I.dtype);
    }
    return S;
}
int stage_block_passes(mtm_ctx* c, const BlockPair& I, const std::vector<BlockPassPlan>& Q, const BlockPassCall& A,
                       BlockPassHost& H) {
    const BlockStage S = pass_stage(c, I, Q, A, H);
    // the mask goes up once, into a buffer of its own, on the call's stream: behind the images, ahead of the gather
    return stage_block_call(c, S, [&]() -> int {
        MTMC(upload_block_pair(c, I));
        if (!A.mask) return MTM_OK;
        MTMC(c->blk_mask.ensure((size_t)I.rows * (size_t)I.cols));
        HIPC(hipMemcpy2DAsync(c->blk_mask.p, (size_t)I.cols, A.mask, (size_t)A.mask_stride_bytes, (size_t)I.cols, (size_t)I.rows,
                              hipMemcpyHostToDevice, c->stream));
        return MTM_OK;
    });
}

// One pass of the chain: its plan and the one that steers it, its rows of the call's device buffers (from the pass's first
// block b0 and tile t0; nullptr: the call has no such row) and what the pass does - every flag derived here, once.
struct BlockPass {
    const BlockPassPlan& q;
    const BlockPassPlan* before;        // the pass whose records steer this one (pass 0: nullptr)
    int np, mode_min;
    BlockTables B;                      // blocks, units (with the constants td) and the fixed tile table
    unsigned long long* keys;
    mtm_hit *recs, *recs2, *steer;
    float* nbhd;
    uint8_t* valid;
    int32_t* pred;
    int32_t* clip;                      // the pass's clip offsets (a call that sums planes; else unused)
    const BlockSecondPass* X;           // (with poff and keys2)
    const mtm_hit* prev;                // the records of `before` that steer this pass: validated or raw
    size_t dtab;                        // the pass's deform tables start at this word of blk_dtab
    bool warped, q8, steers, moved;
};
// row: the first key, record and neighbourhood of the pair the pass runs for (the stack form: every pair has a row of the
// call's blocks; else 0) - the tables and units are the call's, shared by the pairs.
BlockPass block_pass_view(mtm_ctx* c, const std::vector<BlockPassPlan>& Q, const BlockPassCall& A, BlockPassHost& H, size_t p,
                          size_t b0, size_t t0, size_t row = 0) {
    BlockPass V{Q[p], p > 0 ? &Q[p - 1] : nullptr, (int)Q[p].blocks.size(), method_mode_min(A.method) ? 1 : 0,
                ctx_block_tables(c, b0, t0, !A.plan_tiles)};
    // warped: a deformed pass p >= 1 searches the image warped by its steering records' field, over the host's units
    V.warped = A.predicted && p > 0;
    // q8: the field's nodes are Q8 ones, which the pass before left in blk_disp (pass_handover) - else whole pixels
    V.q8 = A.predicted && A.steer;
    // steers: this pass steers another by refined positions, so it needs its neighbourhoods and hands Q8 nodes on
    V.steers = V.q8 && p + 1 < Q.size();
    // moved: blocks_unit_kernel moves the boxes - by the previous pass's records or pass 0's offsets; else the host's units
    V.moved = !V.warped && (p > 0 || A.offsets);
    V.keys = c->blk_keys.as<unsigned long long>() + row + b0;
    V.recs = c->blk_recs.as<mtm_hit>() + row + b0;
    V.nbhd = A.nbhd || V.steers ? c->blk_nbhd.as<float>() + 9 * (row + b0) : nullptr;
    V.clip = c->blk_clip.p ? c->blk_clip.as<int32_t>() + 2 * b0 : nullptr;
    V.valid = A.valid ? c->blk_valid.as<uint8_t>() + b0 : nullptr;
    V.steer = A.valid ? c->blk_steer.as<mtm_hit>() + b0 : nullptr;
    V.pred = A.predicted ? c->blk_pred.as<int32_t>() + 2 * b0 : nullptr;
    V.recs2 = A.second ? c->blk_recs2.as<mtm_hit>() + b0 : nullptr;
    if (A.second) {
        H.X[p].poff = c->blk_poff.as<long long>() + b0;
        H.X[p].keys2 = c->blk_keys2.as<unsigned long long>() + b0;
        V.X = &H.X[p];
    }
    V.prev = p > 0 ? (A.valid ? V.steer : V.recs) - Q[p - 1].blocks.size() : nullptr;
    V.dtab = H.dtab_at[p];
    return V;
}

// What the pass searches, ahead of its chain.  Warped: the steering records become compact displacements
// (deform_disp_kernel; q8: the nodes are already there) and the ORIGINAL image - the stack's slot 1 - is warped by their
// field into blk_warp, *wimg.  Moved: blocks_unit_kernel's units.  Else nothing: the host's units.
// clip != nullptr (a call that sums planes): blocks_unit_clip_kernel, which writes the units' clip offsets there as well.
int pass_search(mtm_ctx* c, const BlockPair& I, const BlockPass& V, ImageDev* wimg, int32_t* clip = nullptr) {
    if (V.warped) {
        const BlockGrid& g = V.before->grid;
        if (!V.q8) MTMC(launch_lanes(c, deform_disp_kernel, V.before->blocks.size(), V.prev, g, c->blk_disp.as<int32_t>()));
        const ImageDev st = image_dev(c);
        MTMC(launch_deform(c, stack_view(st, I.rows, I.rows),
                           c->slot[c->cur].u8b.as<uint8_t>() + st.u8_plane + (size_t)I.rows * st.u8_pitch, I.chans, I.dtype, g,
                           V.dtab, V.q8));
        *wimg = warp_view(c, I.rows, I.cols, I.chans);
    } else if (V.moved && clip) {
        return launch_lanes(c, blocks_unit_clip_kernel, V.np, V.B.blocks, V.np, V.before ? nullptr : c->blk_offs.as<int32_t>(),
                            V.prev, V.before ? V.before->grid : BlockGrid{}, V.q.margin, I.rows, I.cols, V.B.units, clip);
    } else if (V.moved) {
        return launch_lanes(c, blocks_unit_kernel, V.np, V.B.blocks, V.np, V.before ? nullptr : c->blk_offs.as<int32_t>(), V.prev,
                            V.before ? V.before->grid : BlockGrid{}, V.q.margin, I.rows, I.cols, V.B.units);
    }
    return MTM_OK;
}

// The pass's records, behind its chain: blocks_record_kernel decodes the keys; a warped pass adds the field at every
// block's centre (blocks_deform_record_kernel: the record then carries the displacement in the original image, which is
// what validation tests and what steers the next pass); the second keys' records; the median test's flags and steering
// records (np = nx ny: plan_block_passes lays out the whole grid).
int pass_records(mtm_ctx* c, const BlockPassCall& A, const BlockPass& V) {
    const BlockGrid& g = V.q.grid;
    // (a masked call: a block may have no key - second_key_record's (-1, -1) and NaN, the rule its second peaks follow)
    MTMC(launch_lanes(c, A.mask ? blocks_second_record_kernel : blocks_record_kernel, V.np, V.B.units, V.keys, V.B.blocks, V.np,
                      V.mode_min, V.recs));
    if (V.warped)
        MTMC(launch_lanes(c, V.q8 ? blocks_deform_record_kernel<true> : blocks_deform_record_kernel<false>, V.np, V.B.blocks, V.np,
                          V.before->grid, c->blk_disp.as<int32_t>(), V.recs, V.pred));
    if (V.X) MTMC(launch_lanes(c, blocks_second_record_kernel, V.np, V.B.units, V.X->keys2, V.B.blocks, V.np, V.mode_min, V.recs2));
    if (V.valid)        // (4 epsilon: exact)
        MTMC(launch_lanes(c, blocks_validate_kernel, V.np, V.recs, g.nx, g.ny, g.sx, g.sy, A.threshold, 4.0 * A.epsilon, V.valid,
                          V.steer));
    return MTM_OK;
}

// What a pass that steers hands the next: its records, neighbourhoods and flags as Q8 displacements (blocks_steer_q8_kernel),
// filtered into blk_disp (blocks_smooth_q8_kernel) - behind this pass's last reader of blk_disp, which the filter overwrites.
int pass_handover(mtm_ctx* c, const BlockPass& V) {
    if (!V.steers) return MTM_OK;
    const BlockGrid& g = V.q.grid;
    MTMC(launch_lanes(c, blocks_steer_q8_kernel, V.np, V.recs, V.nbhd, V.pred, V.valid, V.steer, g.nx, g.ny, g.sx, g.sy, V.mode_min,
                      c->blk_d8.as<int32_t>()));
    return launch_lanes(c, blocks_smooth_q8_kernel, V.np, c->blk_d8.as<int32_t>(), g.nx, g.ny, c->blk_disp.as<int32_t>());
}

// The chain behind mtm_match_blocks_at / _second (one pass) and the mtm_match_blocks_passes* entries: the stages above per
// pass, in stream order - a pass reads the finished records of the one before -, then what was asked for, behind one wait.
int match_block_passes(mtm_ctx* c, const BlockPair& I, const std::vector<BlockPassPlan>& Q, const BlockPassCall& A) {
    BlockPassHost H;
    MTMC(stage_block_passes(c, I, Q, A, H));
    size_t b0 = 0, t0 = 0;
    for (size_t p = 0; p < Q.size(); ++p) {
        const BlockPass V = block_pass_view(c, Q, A, H, p, b0, t0);
        ImageDev wimg{};
        MTMC(pass_search(c, I, V, &wimg));
        MTMC(blocks_pair(c, V.q.plan, V.B, I.rows, I.chans, I.dtype, A.method, 0, 1, true, BlockSink{V.keys, V.nbhd, 0, 0}, V.X,
                         V.warped ? &wimg : nullptr, V.warped ? wimg.u8 + wimg.u8_plane : nullptr,
                         A.mask ? c->blk_mask.as<uint8_t>() : nullptr));
        MTMC(pass_records(c, A, V));
        MTMC(pass_handover(c, V));
        b0 += V.q.blocks.size();
        t0 += V.q.plan.tiles.size();
    }
    const size_t n = H.blocks.size();
    return finish_block_call(c, {{A.out, c->blk_recs.p, sizeof(mtm_hit) * n}, {A.nbhd, c->blk_nbhd.p, sizeof(float) * 9 * n},
                                 {A.valid, c->blk_valid.p, n}, {A.second, c->blk_recs2.p, sizeof(mtm_hit) * n},
                                 {A.predicted, c->blk_pred.p, sizeof(int32_t) * 2 * n}}, n);
}

// threshold and epsilon of the median test: finite and >= 0, else MTM_E_INVALID naming the argument.
int check_validate_args(const char* who, double threshold, double epsilon) {
    for (const auto& a : {std::make_pair("threshold", threshold), std::make_pair("epsilon", epsilon)})
        if (!(a.second >= 0.0) || !std::isfinite(a.second)) {
            set_error(std::string(who) + ": " + a.first + " must be finite and >= 0 (got " + std::to_string(a.second) + ")");
            return MTM_E_INVALID;
        }
    return MTM_OK;
}

// The preamble of mtm_match_blocks_at / _second behind their record: one pass over the caller's blocks, planned over the
// fixed tile table.  extra_ok: what the entry asks of the arguments that are its own.
int block_single_entry(mtm_ctx* c, const char* who, const BlockPair& I, const mtm_block* blocks, int n_blocks, int margin,
                       bool extra_ok, const BlockPassCall& A) {
    MTMC(check_block_pair(c, who, n_blocks >= 0 && margin >= 0 && extra_ok && (n_blocks == 0 || (blocks && A.out)), A.method, I));
    std::vector<BlockPassPlan> Q(1);
    Q[0].grid = BlockGrid{};
    Q[0].margin = margin;
    MTMC(plan_blocks(I.rows, I.cols, I.chans, I.dtype, blocks, n_blocks, margin, 4 * (long long)c->boxes_max_floats, who, Q[0].plan,
                     A.plan_tiles, A.mask != nullptr));
    if (n_blocks == 0) return MTM_OK;
    if (!A.plan_tiles) MTMC(fix_block_tiles(Q[0].plan, I.rows, I.cols, blocks, margin, who));
    Q[0].blocks.assign(blocks, blocks + n_blocks);
    return match_block_passes(c, I, Q, A);
}

// ... and of the five mtm_match_blocks_passes* entries.  check_median: the median test's arguments are checked - ahead of
// everything else, a null context included.
int block_passes_entry(mtm_ctx* c, const char* who, const BlockPair& I, const mtm_block_pass* passes, int n_passes,
                       bool check_median, bool extra_ok, const BlockPassCall& A) {
    if (check_median) MTMC(check_validate_args(who, A.threshold, A.epsilon));
    MTMC(check_block_pair(c, who, n_passes >= 1 && passes && A.out && extra_ok, A.method, I));
    // deformation: every pass moves a record by less than the image's larger side past the field that steered it
    if (A.predicted && (long long)n_passes * std::max(I.rows, I.cols) > kDeformMaxDisp) {
        set_error(std::string(who) + ": " + std::to_string(n_passes) + " passes over images of this size could pass the "
                  "largest displacement the field takes (2^22 pixels)");
        return MTM_E_INVALID;
    }
    std::vector<BlockPassPlan> Q;
    MTMC(plan_block_passes(I.rows, I.cols, I.chans, I.dtype, passes, n_passes, 4 * (long long)c->boxes_max_floats, who, Q));
    return match_block_passes(c, I, Q, A);
}

// mtm_match_blocks_passes_deformed and mtm_match_blocks_passes_steered - steer = 0: the deformed call, under its name.
int block_deformed_entry(mtm_ctx* c, const char* who, const BlockPair& I, const mtm_block_pass* passes, int n_passes, int method,
                         double threshold, double epsilon, mtm_hit* out, float* nbhd, uint8_t* valid, int32_t* predicted,
                         int steer) {
    BlockPassCall A{method, out, nbhd};
    A.valid = valid, A.threshold = threshold, A.epsilon = epsilon;
    A.predicted = predicted, A.steer = steer;
    return block_passes_entry(c, who, I, passes, n_passes, valid != nullptr, predicted != nullptr, A);
}

// What a debug entry does around its kernels: ensure these buffers, upload those with a source, run(), copy back those
// with a destination, wait.
struct DebugBuf { DevBuf& buf; size_t bytes; const void* src; void* dst; };
template <class Run>
int debug_block_run(mtm_ctx* c, const char* who, std::initializer_list<DebugBuf> bufs, Run&& run) {
    MTM_NOT_IN_FLIGHT(c, who);
    HIPC(hipSetDevice(c->device));
    for (const DebugBuf& b : bufs) MTMC(b.buf.ensure(b.bytes));
    for (const DebugBuf& b : bufs)
        if (b.src) HIPC(hipMemcpyAsync(b.buf.p, b.src, b.bytes, hipMemcpyHostToDevice, c->stream));
    MTMC(run());
    for (const DebugBuf& b : bufs)
        if (b.dst) HIPC(hipMemcpyAsync(b.dst, b.buf.p, b.bytes, hipMemcpyDeviceToHost, c->stream));
    HIPC(hipStreamSynchronize(c->stream));
    return MTM_OK;
}

// ---- the pass chain over a frame stack (mtm_match_blocks_stack_at, mtm_match_blocks_stack_passes)

// The frames of a stack entry point, of one shape, pixel kind and row stride.
struct BlockFrames {
    const void* const* frames;
    int n_frames, rows, cols, chans, dtype;
    int64_t row_stride_bytes;
};

// What both stack-pass entries check behind their own arguments: the frames, and what blocks ask of them.
int check_block_frames(mtm_ctx* c, const char* who, bool args_ok, int method, int mode, const BlockFrames& F) {
    MTMC(check_block_entry(c, who,
                           args_ok && F.n_frames >= 0 && (F.n_frames == 0 || F.frames) &&
                               (mode == MTM_BLOCKS_REF_PREVIOUS || mode == MTM_BLOCKS_REF_FIRST),
                           method));
    for (int f = 0; f < F.n_frames; ++f)
        MTMC(check_image_args(F.frames[f], F.rows, F.cols, F.chans, F.dtype, F.row_stride_bytes, who));
    return check_block_images(who, "frames", F.rows, F.chans, F.dtype);
}

// The planes of the passes Q hold cells[p + 1] - cells[p] floats each, side_p = 2 margin_p + 1; all of them together stay
// within MTM_OPT_BOXES_MAX_FLOATS, else MTM_E_INVALID naming both numbers.
int plan_pass_planes(mtm_ctx* c, const char* who, const std::vector<BlockPassPlan>& Q, std::vector<size_t>& cells) {
    unsigned __int128 total = 0;
    cells.assign(1, 0);
    bool wide = false;
    for (const BlockPassPlan& q : Q) {
        const unsigned __int128 side = 2 * (unsigned __int128)q.margin + 1;
        wide = wide || side > (unsigned __int128)INT_MAX;
        total += (unsigned __int128)q.blocks.size() * side * side;
        cells.push_back((size_t)total);
    }
    if (wide || total > (unsigned __int128)c->boxes_max_floats) {
        const std::string cells_s = total >> 63 ? std::string("2^63 or more") : std::to_string((long long)total);
        set_error(std::string(who) + ": the planes of " + std::to_string(Q.size()) + " pass(es) hold " + cells_s +
                  " floats, more than MTM_OPT_BOXES_MAX_FLOATS = " + std::to_string((long long)c->boxes_max_floats));
        return MTM_E_INVALID;
    }
    return MTM_OK;
}

// match_block_passes over the pairs of a frame stack: the same host tables (pass_stage), views (block_pass_view) and
// launches (pass_search, blocks_pair, pass_records), the frames going up in mtm_match_blocks_stack's chunks
// (plan_blocks_stack) - one host wait.  A.out: the records; A.offsets: pass 0 follows an uploaded displacement.
// Per pair (planes == nullptr): pair r has row r of the call's keys, records and neighbourhoods - n = the blocks of all
// passes, pass-major within the row -, and for every pair of a frame chunk all passes run, each steered by the pair's own
// records of the pass before, ahead of the next upload.  A.out: (n_frames - 1) n records, A.nbhd likewise.
// Ensemble (planes != nullptr): pass after pass - every pair adds to the pass's planes of sums (blocks_plane_fixed_kernel
// at the clip offsets the host planned, pass 0 without offsets, or blocks_unit_clip_kernel computed), then
// blocks_plane_peak_kernel makes the means and the records that steer the next pass.  A pass needs every pair: a stack
// that fits one frame chunk goes up once, any other once per pass.  planes: every pass's, pass-major; A.out: n records.
int match_block_stack_passes(mtm_ctx* c, const BlockFrames& F, const std::vector<BlockPassPlan>& Q, const BlockPassCall& A, int mode,
                             float* planes, const std::vector<size_t>& cells) {
    const BlockPair I{nullptr, 0, nullptr, 0, F.rows, F.cols, F.chans, F.dtype};
    const size_t np = (size_t)F.n_frames - 1;
    const bool ens = planes != nullptr;
    BlockPassHost H;
    BlockStage S = pass_stage(c, I, Q, A, H);
    const size_t n = S.n;
    std::vector<int32_t> clip;
    if (ens) {
        for (const BlockPassPlan& q : Q) clip.insert(clip.end(), q.plan.clip.begin(), q.plan.clip.end());
        S.cells = S.plane_floats = cells.back();
        S.clip = clip.data();
        S.nbhd = false;
    } else {
        S.key_rows = np;
    }
    // the call's clock starts ahead of the uploads: the frames go up chunk by chunk between the pairs' chains
    MTMC(stage_block_call(c, S, [] { return MTM_OK; }));

    const std::vector<StackChunk> chunks = plan_blocks_stack(F.n_frames, track_chunk_frames(c, F.rows, F.cols, F.chans), mode);
    std::vector<const void*> px;
    auto upload = [&](const StackChunk& K) -> int {
        px.assign(1, F.frames[K.carried]);
        px.insert(px.end(), F.frames + K.f0, F.frames + K.f0 + K.nf);
        adopt_image(c, (K.nf + 1) * F.rows, F.cols, F.chans, F.dtype);
        return upload_image_stack(c, c->slot[c->cur], px.data(), K.nf + 1, F.row_stride_bytes, F.rows, F.cols, F.chans, F.dtype,
                                  c->stream);
    };
    auto r_slot = [&](int i) { return mode == MTM_BLOCKS_REF_FIRST ? 0 : i; };
    // one pass, one block chunk, mode "first": the gathered templates outlive the pairs of a frame chunk
    const bool gather_once = mode == MTM_BLOCKS_REF_FIRST && Q.size() == 1 && Q[0].plan.chunks.size() == 1;
    ImageDev none{};
    if (!ens) {
        for (const StackChunk& K : chunks) {
            MTMC(upload(K));
            for (int i = 0; i < K.nf; ++i) {
                const size_t pair = (size_t)(K.p0 + i);
                size_t b0 = 0, t0 = 0;
                for (size_t p = 0; p < Q.size(); ++p) {
                    const BlockPass V = block_pass_view(c, Q, A, H, p, b0, t0, pair * n);
                    // (uploaded offsets move pass 0's boxes alike for every pair: once)
                    if (p > 0 || pair == 0) MTMC(pass_search(c, I, V, &none));
                    MTMC(blocks_pair(c, V.q.plan, V.B, F.rows, F.chans, F.dtype, A.method, r_slot(i), i + 1,
                                     !(gather_once && i > 0), BlockSink{V.keys, V.nbhd, 0, 0}));
                    MTMC(pass_records(c, A, V));
                    b0 += V.q.blocks.size();
                    t0 += V.q.plan.tiles.size();
                }
            }
        }
        return finish_block_call(c, {{A.out, c->blk_recs.p, sizeof(mtm_hit) * np * n},
                                     {A.nbhd, c->blk_nbhd.p, sizeof(float) * 9 * np * n}}, np * n);
    }
    const bool resident = chunks.size() == 1;
    if (resident) MTMC(upload(chunks[0]));
    size_t b0 = 0, t0 = 0;
    for (size_t p = 0; p < Q.size(); ++p) {
        const BlockPass V = block_pass_view(c, Q, A, H, p, b0, t0);
        const int side = 2 * V.q.margin + 1;
        double* acc = c->blk_acc.as<double>() + cells[p];
        MTMC(pass_search(c, I, V, &none, V.clip));
        for (const StackChunk& K : chunks) {
            if (!resident) MTMC(upload(K));
            for (int i = 0; i < K.nf; ++i)
                MTMC(blocks_pair(c, V.q.plan, V.B, F.rows, F.chans, F.dtype, A.method, r_slot(i), i + 1, !(gather_once && i > 0),
                                 BlockSink{nullptr, nullptr, side, K.p0 + i == 0 ? 1 : 0, acc, V.clip}));
        }
        MTMC(for_launch_slices(0, (size_t)V.np, [&](size_t k0, unsigned nk) -> int {
            hipLaunchKernelGGL(blocks_plane_peak_kernel, dim3(nk), dim3(256), 0, c->stream, acc, V.B.units, V.clip, V.B.blocks,
                               (int)k0, side, (double)np, V.mode_min, c->blk_plane.as<float>() + cells[p], V.recs);
            HIPC(hipGetLastError());
            return MTM_OK;
        }));
        b0 += V.q.blocks.size();
        t0 += V.q.plan.tiles.size();
    }
    return finish_block_call(c, {{planes, c->blk_plane.p, sizeof(float) * cells.back()}, {A.out, c->blk_recs.p, sizeof(mtm_hit) * n}},
                             n);
}

}  // namespace

extern "C" {

int mtm_match_blocks_stack_at(mtm_ctx* c, const void* const* frames, int n_frames, int rows, int cols, int chans, int dtype,
                              int64_t row_stride_bytes, const mtm_block* blocks, const int32_t* offsets, int n_blocks, int margin,
                              int method, int mode, mtm_hit* out_hits, float* nbhd, float* planes) {
    const char* who = "mtm_match_blocks_stack_at";
    const BlockFrames F{frames, n_frames, rows, cols, chans, dtype, row_stride_bytes};
    MTMC(check_block_frames(c, who,
                            n_blocks >= 0 && margin >= 0 &&
                                (n_blocks == 0 || (blocks && offsets && n_frames >= 2 && (out_hits || planes))),
                            method, mode, F));
    std::vector<BlockPassPlan> Q(1);
    Q[0].grid = BlockGrid{};
    Q[0].margin = margin;
    MTMC(plan_blocks(rows, cols, chans, dtype, blocks, n_blocks, margin, 4 * (long long)c->boxes_max_floats, who, Q[0].plan, false));
    if (n_blocks == 0) return MTM_OK;
    MTMC(fix_block_tiles(Q[0].plan, rows, cols, blocks, margin, who));
    Q[0].blocks.assign(blocks, blocks + n_blocks);
    std::vector<size_t> cells;
    if (planes) MTMC(plan_pass_planes(c, who, Q, cells));
    BlockPassCall A{method, out_hits, planes ? nullptr : nbhd};
    A.offsets = offsets;
    return match_block_stack_passes(c, F, Q, A, mode, planes, cells);
}

int mtm_match_blocks_stack_passes(mtm_ctx* c, const void* const* frames, int n_frames, int rows, int cols, int chans, int dtype,
                                  int64_t row_stride_bytes, const mtm_block_pass* passes, int n_passes, int method, int mode,
                                  mtm_hit* out_hits, float* nbhd, float* planes) {
    const char* who = "mtm_match_blocks_stack_passes";
    const BlockFrames F{frames, n_frames, rows, cols, chans, dtype, row_stride_bytes};
    MTMC(check_block_frames(c, who, n_passes >= 1 && passes && n_frames >= 2 && (out_hits || planes), method, mode, F));
    std::vector<BlockPassPlan> Q;
    MTMC(plan_block_passes(rows, cols, chans, dtype, passes, n_passes, 4 * (long long)c->boxes_max_floats, who, Q));
    std::vector<size_t> cells;
    if (planes) MTMC(plan_pass_planes(c, who, Q, cells));
    return match_block_stack_passes(c, F, Q, BlockPassCall{method, out_hits, planes ? nullptr : nbhd}, mode, planes, cells);
}

int mtm_debug_plane_peaks(mtm_ctx* c, const double* acc, int n, int side, const int32_t* clip, const int32_t* oh,
                          const int32_t* ow, int pairs, int method, float* planes_out, mtm_hit* recs_out) {
    const char* who = "mtm_debug_plane_peaks";
    bool ok = acc && clip && oh && ow && planes_out && recs_out && n >= 1 && side >= 1 && side % 2 == 1 && pairs >= 1 &&
              method >= MTM_TM_SQDIFF && method <= MTM_TM_CCOEFF_NORMED && (long long)side * side * n <= INT_MAX;
    for (int k = 0; ok && k < n; ++k)
        ok = oh[k] >= 0 && ow[k] >= 0 && oh[k] <= side && ow[k] <= side && clip[2 * k] >= 0 && clip[2 * k + 1] >= 0 &&
             clip[2 * k] <= side && clip[2 * k + 1] <= side;
    if (!ok) {
        set_error(std::string(who) + ": bad arguments");
        return MTM_E_INVALID;
    }
    const int mode_min = method_mode_min(method) ? 1 : 0, m = side / 2;
    const size_t nn = (size_t)n, cells = (size_t)side * (size_t)side;
    // block k: a unit whose plane is centred on displacement (0, 0) - the records carry (dx, dy)
    std::vector<TrackUnit> units(nn);
    for (int k = 0; k < n; ++k) units[(size_t)k] = TrackUnit{k, clip[2 * k + 1] - m, clip[2 * k] - m, oh[k], ow[k]};
    if (!c) {           // the rule itself, on the host
        for (size_t k = 0; k < nn; ++k) {
            const TrackUnit& U = units[k];
            const int ox = clip[2 * k], oy = clip[2 * k + 1];
            unsigned long long best = 0ull;
            for (size_t idx = 0; idx < cells; ++idx) {
                const int y = (int)(idx / (size_t)side) - oy, x = (int)(idx % (size_t)side) - ox;
                const bool in = y >= 0 && y < U.oh && x >= 0 && x < U.ow;
                const float v = in ? (float)(acc[k * cells + idx] / (double)pairs) : NAN;
                planes_out[k * cells + idx] = v;
                const unsigned long long key = second_cell_key(v, mode_min, (uint32_t)idx);
                best = key > best ? key : best;
            }
            recs_out[k] = best ? key_record(key_index(best), planes_out[k * cells + key_index(best)], (int)k, U.y0 - oy, U.x0 - ox,
                                            side, 0, 0)
                               : second_key_record(0ull, mode_min, (int)k, 0, 0, side, 0, 0);
        }
        return MTM_OK;
    }
    const std::vector<mtm_block> blocks(nn, mtm_block{0, 0, 0, 0});
    return debug_block_run(
        c, who,
        {{c->blk_acc, sizeof(double) * nn * cells, acc, nullptr}, {c->blk_clip, sizeof(int32_t) * 2 * nn, clip, nullptr},
         {c->blk_units, sizeof(TrackUnit) * nn, units.data(), nullptr}, {c->blk_blocks, sizeof(mtm_block) * nn, blocks.data(), nullptr},
         {c->blk_plane, sizeof(float) * nn * cells, nullptr, planes_out}, {c->blk_recs, sizeof(mtm_hit) * nn, nullptr, recs_out}},
        [&]() -> int {
            return for_launch_slices(0, nn, [&](size_t k0, unsigned nk) -> int {
                hipLaunchKernelGGL(blocks_plane_peak_kernel, dim3(nk), dim3(256), 0, c->stream, c->blk_acc.as<double>(),
                                   c->blk_units.as<TrackUnit>(), c->blk_clip.as<int32_t>(), c->blk_blocks.as<mtm_block>(), (int)k0,
                                   side, (double)pairs, mode_min, c->blk_plane.as<float>(), c->blk_recs.as<mtm_hit>());
                HIPC(hipGetLastError());
                return MTM_OK;
            });
        });
}

int mtm_match_blocks_at(mtm_ctx* c, const void* reference, int64_t reference_stride_bytes, const void* image,
                        int64_t image_stride_bytes, int rows, int cols, int chans, int dtype, const mtm_block* blocks,
                        const int32_t* offsets, int n_blocks, int margin, int method, mtm_hit* out, float* nbhd) {
    BlockPassCall A{method, out, nbhd};
    A.offsets = offsets;
    return block_single_entry(c, "mtm_match_blocks_at",
                              {reference, reference_stride_bytes, image, image_stride_bytes, rows, cols, chans, dtype}, blocks,
                              n_blocks, margin, n_blocks == 0 || offsets, A);
}

int mtm_match_blocks_second(mtm_ctx* c, const void* reference, int64_t reference_stride_bytes, const void* image,
                            int64_t image_stride_bytes, int rows, int cols, int chans, int dtype, const mtm_block* blocks,
                            const int32_t* offsets, int n_blocks, int margin, int method, mtm_hit* out, float* nbhd,
                            int exclusion, mtm_hit* second) {
    BlockPassCall A{method, out, nbhd};
    A.offsets = offsets, A.second = second, A.exclusion = exclusion;
    return block_single_entry(c, "mtm_match_blocks_second",
                              {reference, reference_stride_bytes, image, image_stride_bytes, rows, cols, chans, dtype}, blocks,
                              n_blocks, margin, exclusion >= 0 && second, A);
}

int mtm_match_blocks_masked(mtm_ctx* c, const void* reference, int64_t reference_stride_bytes, const void* image,
                            int64_t image_stride_bytes, const void* mask, int64_t mask_stride_bytes, int rows, int cols, int chans,
                            int dtype, const mtm_block* blocks, int n_blocks, const int32_t* offsets, int margin, int method,
                            int exclusion, mtm_hit* out, float* nbhd, mtm_hit* second) {
    const char* who = "mtm_match_blocks_masked";
    const char* bad = !mask ? "mask is NULL"
                      : dtype != MTM_U8 ? "dtype: a masked call takes uint8 images"
                      : method != MTM_TM_SQDIFF && method != MTM_TM_CCORR_NORMED
                          ? "method: a masked call takes TM_SQDIFF (0) and TM_CCORR_NORMED (3)"
                      : cols >= 1 && mask_stride_bytes < (int64_t)cols ? "mask_stride_bytes is below cols" : nullptr;
    if (bad) {
        set_error(std::string(who) + ": " + bad);
        return MTM_E_INVALID;
    }
    BlockPassCall A{method, out, nbhd};
    A.offsets = offsets, A.mask = mask, A.mask_stride_bytes = mask_stride_bytes;
    if (exclusion >= 0) A.second = second, A.exclusion = exclusion;
    A.plan_tiles = !offsets && exclusion < 0;
    return block_single_entry(c, who, {reference, reference_stride_bytes, image, image_stride_bytes, rows, cols, chans, dtype},
                              blocks, n_blocks, margin, exclusion < 0 || second, A);
}

int mtm_match_blocks_passes(mtm_ctx* c, const void* reference, int64_t reference_stride_bytes, const void* image,
                            int64_t image_stride_bytes, int rows, int cols, int chans, int dtype,
                            const mtm_block_pass* passes, int n_passes, int method, mtm_hit* out, float* nbhd) {
    return block_passes_entry(c, "mtm_match_blocks_passes",
                              {reference, reference_stride_bytes, image, image_stride_bytes, rows, cols, chans, dtype}, passes,
                              n_passes, /* check_median */ false, /* extra_ok */ true, BlockPassCall{method, out, nbhd});
}

int mtm_match_blocks_passes_validated(mtm_ctx* c, const void* reference, int64_t reference_stride_bytes, const void* image,
                                      int64_t image_stride_bytes, int rows, int cols, int chans, int dtype,
                                      const mtm_block_pass* passes, int n_passes, int method, double threshold,
                                      double epsilon, mtm_hit* out, float* nbhd, uint8_t* valid) {
    BlockPassCall A{method, out, nbhd};
    A.valid = valid, A.threshold = threshold, A.epsilon = epsilon;
    return block_passes_entry(c, "mtm_match_blocks_passes_validated",
                              {reference, reference_stride_bytes, image, image_stride_bytes, rows, cols, chans, dtype}, passes,
                              n_passes, /* check_median */ true, valid != nullptr, A);
}

int mtm_match_blocks_passes_second(mtm_ctx* c, const void* reference, int64_t reference_stride_bytes, const void* image,
                                   int64_t image_stride_bytes, int rows, int cols, int chans, int dtype,
                                   const mtm_block_pass* passes, int n_passes, int method, double threshold, double epsilon,
                                   mtm_hit* out, float* nbhd, uint8_t* valid, int exclusion, mtm_hit* second) {
    BlockPassCall A{method, out, nbhd};
    A.valid = valid, A.threshold = threshold, A.epsilon = epsilon;
    A.second = second, A.exclusion = exclusion;
    return block_passes_entry(c, "mtm_match_blocks_passes_second",
                              {reference, reference_stride_bytes, image, image_stride_bytes, rows, cols, chans, dtype}, passes,
                              n_passes, valid != nullptr, exclusion >= 0 && second, A);
}

int mtm_match_blocks_passes_deformed(mtm_ctx* c, const void* reference, int64_t reference_stride_bytes, const void* image,
                                     int64_t image_stride_bytes, int rows, int cols, int chans, int dtype,
                                     const mtm_block_pass* passes, int n_passes, int method, double threshold, double epsilon,
                                     mtm_hit* out, float* nbhd, uint8_t* valid, int32_t* predicted) {
    return block_deformed_entry(c, "mtm_match_blocks_passes_deformed",
                                {reference, reference_stride_bytes, image, image_stride_bytes, rows, cols, chans, dtype}, passes,
                                n_passes, method, threshold, epsilon, out, nbhd, valid, predicted, 0);
}

int mtm_match_blocks_passes_steered(mtm_ctx* c, const void* reference, int64_t reference_stride_bytes, const void* image,
                                    int64_t image_stride_bytes, int rows, int cols, int chans, int dtype,
                                    const mtm_block_pass* passes, int n_passes, int method, double threshold, double epsilon,
                                    mtm_hit* out, float* nbhd, uint8_t* valid, int32_t* predicted, int steer) {
    if (steer != 0 && steer != 1) {
        set_error(std::string("mtm_match_blocks_passes_steered: steer must be 0 (integer records) or 1 (refined positions) (got ") +
                  std::to_string(steer) + ")");
        return MTM_E_INVALID;
    }
    return block_deformed_entry(c, steer ? "mtm_match_blocks_passes_steered" : "mtm_match_blocks_passes_deformed",
                                {reference, reference_stride_bytes, image, image_stride_bytes, rows, cols, chans, dtype}, passes,
                                n_passes, method, threshold, epsilon, out, nbhd, valid, predicted, steer);
}

int mtm_debug_validate_blocks(mtm_ctx* c, const mtm_hit* recs, int nx, int ny, int sx, int sy, double threshold, double epsilon,
                              uint8_t* valid, mtm_hit* steer) {
    const char* who = "mtm_debug_validate_blocks";
    if (!recs || !valid || !steer || nx < 1 || ny < 1 || sx < 1 || sy < 1 || (long long)nx * ny > INT_MAX) {
        set_error(std::string(who) + ": bad arguments");
        return MTM_E_INVALID;
    }
    MTMC(check_validate_args(who, threshold, epsilon));
    const size_t n = (size_t)nx * (size_t)ny;
    const double e4 = 4.0 * epsilon;
    if (!c) {           // the rule itself, on the host
        for (int k = 0; k < (int)n; ++k)
            valid[k] = blocks_steer_record_inl(recs, nx, ny, sx, sy, k, threshold, e4, &steer[k]) ? 1 : 0;
        return MTM_OK;
    }
    return debug_block_run(c, who, {{c->blk_recs, sizeof(mtm_hit) * n, recs, nullptr}, {c->blk_valid, n, nullptr, valid},
                                    {c->blk_steer, sizeof(mtm_hit) * n, nullptr, steer}}, [&] {
        return launch_lanes(c, blocks_validate_kernel, n, c->blk_recs.as<mtm_hit>(), nx, ny, sx, sy, threshold, e4,
                            c->blk_valid.as<uint8_t>(), c->blk_steer.as<mtm_hit>());
    });
}

int mtm_debug_steer_q8(mtm_ctx* c, const mtm_hit* recs, const float* nbhd, const int32_t* predicted, const uint8_t* valid,
                       const mtm_hit* steer_recs, int nx, int ny, int sx, int sy, int mode_min, int smooth, int32_t* out_q8) {
    const char* who = "mtm_debug_steer_q8";
    if (!recs || !nbhd || !predicted || !out_q8 || (valid != nullptr) != (steer_recs != nullptr) || nx < 1 || ny < 1 || sx < 1 ||
        sy < 1 || (long long)nx * ny > INT_MAX / 16) {
        set_error(std::string(who) + ": bad arguments");
        return MTM_E_INVALID;
    }
    const size_t n = (size_t)nx * (size_t)ny;
    mode_min = mode_min ? 1 : 0;
    if (!c) {           // the rule itself, on the host
        std::vector<int32_t> d8(2 * n);
        for (int k = 0; k < (int)n; ++k)
            steer_d8_inl(recs, nbhd, predicted, valid, steer_recs, nx, sx, sy, mode_min, k, &d8[2 * (size_t)k], &d8[2 * (size_t)k + 1]);
        for (int k = 0; k < (int)n; ++k) {
            if (smooth) steer_smooth_inl(d8.data(), nx, ny, k % nx, k / nx, &out_q8[2 * (size_t)k], &out_q8[2 * (size_t)k + 1]);
            else out_q8[2 * (size_t)k] = d8[2 * (size_t)k], out_q8[2 * (size_t)k + 1] = d8[2 * (size_t)k + 1];
        }
        return MTM_OK;
    }
    const size_t rb = sizeof(mtm_hit) * n, pairs = sizeof(int32_t) * 2 * n;
    return debug_block_run(
        c, who,
        {{c->blk_valid, valid ? n : 0, valid, nullptr}, {c->blk_steer, valid ? rb : 0, steer_recs, nullptr},
         {c->blk_recs, rb, recs, nullptr}, {c->blk_nbhd, sizeof(float) * 9 * n, nbhd, nullptr},
         {c->blk_pred, pairs, predicted, nullptr}, {c->blk_d8, pairs, nullptr, smooth ? nullptr : out_q8},
         {c->blk_disp, pairs, nullptr, smooth ? out_q8 : nullptr}},
        [&]() -> int {
            MTMC(launch_lanes(c, blocks_steer_q8_kernel, n, c->blk_recs.as<mtm_hit>(), c->blk_nbhd.as<float>(),
                              c->blk_pred.as<int32_t>(), valid ? c->blk_valid.as<uint8_t>() : nullptr,
                              valid ? c->blk_steer.as<mtm_hit>() : nullptr, nx, ny, sx, sy, mode_min, c->blk_d8.as<int32_t>()));
            if (!smooth) return MTM_OK;
            return launch_lanes(c, blocks_smooth_q8_kernel, n, c->blk_d8.as<int32_t>(), nx, ny, c->blk_disp.as<int32_t>());
        });
}


// mtm_deform_image (q8 = false: whole-pixel displacements within +-2^22) and mtm_deform_image_q8 (Q8 ones within +-2^30).
static int deform_image_entry(const char* who, bool q8, mtm_ctx* c, const void* px, int64_t row_stride_bytes, int rows, int cols,
                              int chans, int dtype, int bw, int bh, int sx, int sy, const int32_t* displacements, void* out,
                              int64_t out_stride_bytes) {
    if (!displacements || !out) {
        set_error(std::string(who) + ": bad arguments");
        return MTM_E_INVALID;
    }
    MTMC(check_image_args(px, rows, cols, chans, dtype, row_stride_bytes, who));
    MTMC(check_image_args(out, rows, cols, chans, dtype, out_stride_bytes, who));
    if (!((dtype == MTM_U8 && (chans == 1 || chans == 3)) || (dtype == MTM_U16 && chans == 1)) || rows > kBatchMaxRows) {
        set_error(std::string(who) + ": takes uint8 images with 1 or 3 channels and single-channel uint16 images of at most " +
                  std::to_string(kBatchMaxRows) + " rows");
        return MTM_E_INVALID;
    }
    const BlockGrid g = block_grid_of(mtm_block_pass{bw, bh, sx, sy, 0}, rows, cols);
    if (g.nx < 1 || g.ny < 1 || (long long)g.nx * g.ny > INT_MAX / 2) {
        set_error(std::string(who) + ": block and step must be >= 1 and a block must fit the image (fewer than 2^30 of them)");
        return MTM_E_INVALID;
    }
    const size_t n = (size_t)g.nx * (size_t)g.ny;
    const long long dmax = q8 ? kDeformMaxDispQ8 : kDeformMaxDisp;
    for (size_t k = 0; k < 2 * n; ++k)
        if (displacements[k] > dmax || displacements[k] < -dmax) {
            set_error(std::string(who) + ": block " + std::to_string(k / 2) + ": displacement beyond 2^22 pixels");
            return MTM_E_INVALID;
        }
    const size_t es = elem_size(dtype);
    if (!c) {           // the rule itself, on the host
        for (int y = 0; y < rows; ++y) {
            uint8_t* orow = (uint8_t*)out + (size_t)y * (size_t)out_stride_bytes;
            for (int x = 0; x < cols; ++x) {
                long long fx, fy;
                if (q8) deform_field_at_of_inl<true>(g, displacements, 2ll * x, 2ll * y, &fx, &fy);
                else deform_field_at_inl(g, displacements, 2ll * x, 2ll * y, &fx, &fy);
                int x0, x1, wx, y0, y1, wy;
                deform_sample_inl(x, fx, cols, &x0, &x1, &wx);
                deform_sample_inl(y, fy, rows, &y0, &y1, &wy);
                const uint8_t* r0 = (const uint8_t*)px + (size_t)y0 * (size_t)row_stride_bytes;
                const uint8_t* r1 = (const uint8_t*)px + (size_t)y1 * (size_t)row_stride_bytes;
                for (int ch = 0; ch < chans; ++ch) {
                    auto at = [&](const uint8_t* r, int xx) -> uint32_t {
                        const size_t e = (size_t)xx * chans + ch;
                        return es == 2 ? (uint32_t)((const uint16_t*)r)[e] : (uint32_t)r[e];
                    };
                    const uint32_t v = deform_blend_inl(at(r0, x0), at(r0, x1), at(r1, x0), at(r1, x1), wx, wy);
                    const size_t e = (size_t)x * chans + ch;
                    if (es == 2) ((uint16_t*)orow)[e] = (uint16_t)v;
                    else orow[e] = (uint8_t)v;
                }
            }
        }
        return MTM_OK;
    }
    MTM_NOT_IN_FLIGHT(c, who);
    HIPC(hipSetDevice(c->device));
    std::vector<uint32_t> tab;
    deform_tables(g, rows, cols, tab);
    const int pitch = (int)round_up((size_t)cols + kPadCols, 64);
    const size_t wbytes = warp_bytes(rows, pitch, chans, dtype);
    MTMC(c->blk_disp.ensure(sizeof(int32_t) * 2 * n));
    MTMC(c->blk_dtab.ensure(sizeof(uint32_t) * tab.size()));
    MTMC(c->blk_warp.ensure(wbytes));
    c->timing = mtm_timing{};
    c->maps_valid = false;
    c->last_hits.clear();
    // ONE upload of the image; the warp reads its planes and writes planes of the same layout
    MTMC(upload_image(c, c->slot[c->cur], px, row_stride_bytes, rows, cols, chans, dtype, c->stream, 1));
    adopt_image(c, rows, cols, chans, dtype);
    HIPC(hipMemcpyAsync(c->blk_disp.p, displacements, sizeof(int32_t) * 2 * n, hipMemcpyHostToDevice, c->stream));
    HIPC(hipMemcpyAsync(c->blk_dtab.p, tab.data(), sizeof(uint32_t) * tab.size(), hipMemcpyHostToDevice, c->stream));
    const ImageDev src = image_dev(c);
    HIPC(hipEventRecord(c->ev[0], c->stream));                  // (the call's time is the warp kernel's)
    MTMC(launch_deform(c, src, c->slot[c->cur].u8b.as<uint8_t>() + src.u8_plane, chans, dtype, g, 0, q8));
    HIPC(hipEventRecord(c->ev[1], c->stream));
    // the planes come back tightly packed; interleaved pixels are put together on the host
    const int np = dtype == MTM_U16 ? 2 : chans;
    const bool direct = np == 1;
    std::vector<uint8_t> planes(direct ? 0 : (size_t)np * rows * cols);
    for (int p = 0; p < np; ++p)
        HIPC(hipMemcpy2DAsync(direct ? out : (void*)(planes.data() + (size_t)p * rows * cols),
                              direct ? (size_t)out_stride_bytes : (size_t)cols, c->blk_warp.as<uint8_t>() + (size_t)p * pitch * rows,
                              (size_t)pitch, (size_t)cols, (size_t)rows, hipMemcpyDeviceToHost, c->stream));
    HIPC(hipStreamSynchronize(c->stream));
    HIPC(hipEventElapsedTime(&c->timing.total_ms, c->ev[0], c->ev[1]));
    const size_t plane = (size_t)rows * cols;
    for (int y = 0; !direct && y < rows; ++y) {
        uint8_t* orow = (uint8_t*)out + (size_t)y * (size_t)out_stride_bytes;
        const uint8_t* q = planes.data() + (size_t)y * cols;
        for (int x = 0; x < cols; ++x) {
            if (dtype == MTM_U16) ((uint16_t*)orow)[x] = (uint16_t)(((uint32_t)q[x] << 8) | ((uint32_t)q[plane + x] ^ 0x80u));
            else
                for (int ch = 0; ch < chans; ++ch) orow[(size_t)x * chans + ch] = q[(size_t)ch * plane + x];
        }
    }
    return MTM_OK;
}

int mtm_deform_image(mtm_ctx* c, const void* px, int64_t row_stride_bytes, int rows, int cols, int chans, int dtype, int bw, int bh,
                     int sx, int sy, const int32_t* displacements, void* out, int64_t out_stride_bytes) {
    return deform_image_entry("mtm_deform_image", false, c, px, row_stride_bytes, rows, cols, chans, dtype, bw, bh, sx, sy,
                              displacements, out, out_stride_bytes);
}

int mtm_deform_image_q8(mtm_ctx* c, const void* px, int64_t row_stride_bytes, int rows, int cols, int chans, int dtype, int bw,
                        int bh, int sx, int sy, const int32_t* displacements_q8, void* out, int64_t out_stride_bytes) {
    return deform_image_entry("mtm_deform_image_q8", true, c, px, row_stride_bytes, rows, cols, chans, dtype, bw, bh, sx, sy,
                              displacements_q8, out, out_stride_bytes);
}

int mtm_debug_second_peaks(mtm_ctx* c, const float* planes, int n, const int32_t* oh, const int32_t* ow, const int32_t* firsts,
                           int mode_min, int exclusion, mtm_hit* out) {
    const char* who = "mtm_debug_second_peaks";
    bool ok = planes && oh && ow && out && n >= 1 && exclusion >= 0 && (mode_min == 0 || mode_min == 1);
    std::vector<long long> poff;
    size_t total = 0;
    for (int k = 0; ok && k < n; ++k) {
        ok = oh[k] >= 1 && ow[k] >= 1 && (long long)oh[k] * ow[k] < (1ll << 32) &&
             (!firsts || (firsts[k] >= 0 && (long long)firsts[k] < (long long)oh[k] * ow[k]));
        poff.push_back((long long)total);
        if (ok) total += (size_t)oh[k] * (size_t)ow[k];
    }
    if (!ok) {
        set_error(std::string(who) + ": bad arguments");
        return MTM_E_INVALID;
    }
    // the first peak of every plane: the cell the caller names, or the largest key of the plane (0: a plane of NaNs)
    std::vector<unsigned long long> first((size_t)n);
    for (int k = 0; k < n; ++k) {
        const float* m = planes + poff[(size_t)k];
        first[(size_t)k] = firsts ? second_cell_key(m[firsts[k]], mode_min, (uint32_t)firsts[k])
                                  : second_scan_inl(m, oh[k], ow[k], 0ull, mode_min, 0);
    }
    if (!c) {           // the rule itself, on the host
        for (int k = 0; k < n; ++k) {
            const unsigned long long f = first[(size_t)k];
            const unsigned long long key2 = f ? second_scan_inl(planes + poff[(size_t)k], oh[k], ow[k], f, mode_min, exclusion) : 0ull;
            out[k] = second_key_record(key2, mode_min, k, 0, 0, ow[k], 0, 0);
        }
        return MTM_OK;
    }
    std::vector<TrackUnit> units((size_t)n);
    for (int k = 0; k < n; ++k) units[(size_t)k] = TrackUnit{k, 0, 0, oh[k], ow[k]};
    const std::vector<mtm_block> blocks((size_t)n, mtm_block{0, 0, 0, 0});
    const size_t nn = (size_t)n;
    const size_t kb = sizeof(unsigned long long) * nn;
    return debug_block_run(
        c, who,
        {{c->blk_plane, sizeof(float) * total, planes, nullptr}, {c->blk_poff, sizeof(long long) * nn, poff.data(), nullptr},
         {c->blk_units, sizeof(TrackUnit) * nn, units.data(), nullptr}, {c->blk_blocks, sizeof(mtm_block) * nn, blocks.data(), nullptr},
         {c->blk_keys, kb, first.data(), nullptr}, {c->blk_keys2, kb, nullptr, nullptr},
         {c->blk_recs2, sizeof(mtm_hit) * nn, nullptr, out}},
        [&]() -> int {
            MTMC(for_launch_slices(0, nn, [&](size_t k0, unsigned nk) -> int {
                hipLaunchKernelGGL(blocks_second_kernel, dim3(nk), dim3(256), 0, c->stream, c->blk_units.as<TrackUnit>(),
                                   c->blk_keys.as<unsigned long long>(), c->blk_plane.as<float>(), c->blk_poff.as<long long>(),
                                   (int)k0, mode_min, exclusion, c->blk_keys2.as<unsigned long long>());
                HIPC(hipGetLastError());
                return MTM_OK;
            }));
            return launch_lanes(c, blocks_second_record_kernel, nn, c->blk_units.as<TrackUnit>(),
                                c->blk_keys2.as<unsigned long long>(), c->blk_blocks.as<mtm_block>(), n, mode_min,
                                c->blk_recs2.as<mtm_hit>());
        });
}


int mtm_match_blocks(mtm_ctx* c, const void* reference, int64_t reference_stride_bytes, const void* image,
                     int64_t image_stride_bytes, int rows, int cols, int chans, int dtype, const mtm_block* blocks,
                     int n_blocks, int margin, int method, mtm_hit* out, float* nbhd) {
    const char* who = "mtm_match_blocks";
    const BlockPair I{reference, reference_stride_bytes, image, image_stride_bytes, rows, cols, chans, dtype};
    MTMC(check_block_pair(c, who, n_blocks >= 0 && margin >= 0 && (n_blocks == 0 || (blocks && out)), method, I));
    BlockPlan P;
    MTMC(plan_blocks(rows, cols, chans, dtype, blocks, n_blocks, margin, 4 * (long long)c->boxes_max_floats, who, P));
    if (n_blocks == 0) return MTM_OK;
    const size_t n = (size_t)n_blocks;

    BlockStage S = plan_stage(blocks, P);
    S.nbhd = nbhd != nullptr;
    MTMC(stage_block_call(c, S, [&] { return upload_block_pair(c, I); }));
    unsigned long long* keys = c->blk_keys.as<unsigned long long>();
    MTMC(blocks_pair(c, P, ctx_block_tables(c), rows, chans, dtype, method, 0, 1, true,
                     BlockSink{keys, nbhd ? c->blk_nbhd.as<float>() : nullptr, 0, 0}));

    // the keys (and neighbourhoods) come back behind the call's single wait
    std::vector<unsigned long long> hkeys(n);
    MTMC(finish_block_call(c, {{hkeys.data(), keys, sizeof(unsigned long long) * n}, {nbhd, c->blk_nbhd.p, sizeof(float) * 9 * n}},
                           n));
    decode_block_keys(P, blocks, hkeys.data(), method, out);
    return MTM_OK;
}

int mtm_match_blocks_stack(mtm_ctx* c, const void* const* frames, int n_frames, int rows, int cols, int chans, int dtype,
                           int64_t row_stride_bytes, const mtm_block* blocks, int n_blocks, int margin, int method, int mode,
                           mtm_hit* out_hits, float* nbhd, float* planes) {
    const char* who = "mtm_match_blocks_stack";
    MTMC(check_block_entry(c, who,
                           n_frames >= 0 && n_blocks >= 0 && margin >= 0 && (n_frames == 0 || frames) &&
                               (n_blocks == 0 || (blocks && n_frames >= 2 && (out_hits || planes))) &&
                               (mode == MTM_BLOCKS_REF_PREVIOUS || mode == MTM_BLOCKS_REF_FIRST),
                           method));
    for (int f = 0; f < n_frames; ++f) MTMC(check_image_args(frames[f], rows, cols, chans, dtype, row_stride_bytes, who));
    MTMC(check_block_images(who, "frames", rows, chans, dtype));
    BlockPlan P;
    MTMC(plan_blocks(rows, cols, chans, dtype, blocks, n_blocks, margin, 4 * (long long)c->boxes_max_floats, who, P));
    if (n_blocks == 0) return MTM_OK;
    const bool ens = planes != nullptr;
    if (ens) nbhd = nullptr;
    const size_t n = (size_t)n_blocks, np = (size_t)n_frames - 1;
    const unsigned __int128 side = 2 * (unsigned __int128)margin + 1, cells128 = (unsigned __int128)n * side * side;
    if (ens && (cells128 > (unsigned __int128)c->boxes_max_floats || side > (unsigned __int128)INT_MAX)) {
        const std::string cells_s = cells128 >> 63 ? std::string("2^63 or more") : std::to_string((long long)cells128);
        set_error(std::string(who) + ": the planes of " + std::to_string(n_blocks) + " blocks at margin " +
                  std::to_string(margin) + " hold " + cells_s + " floats, more than MTM_OPT_BOXES_MAX_FLOATS = " +
                  std::to_string((long long)c->boxes_max_floats));
        return MTM_E_INVALID;
    }
    const size_t cells = ens ? (size_t)cells128 : 0;

    // the call's clock starts ahead of the uploads: the frames go up chunk by chunk between the pairs' chains
    BlockStage S = plan_stage(blocks, P);
    S.key_rows = np;
    S.nbhd = nbhd != nullptr;
    S.cells = cells;
    S.clip = ens ? P.clip.data() : nullptr;
    MTMC(stage_block_call(c, S, [] { return MTM_OK; }));

    // mode "first" with every block in one chunk: the gathered templates outlive the pairs of a frame chunk
    const bool gather_once = mode == MTM_BLOCKS_REF_FIRST && P.chunks.size() == 1;
    std::vector<const void*> px;
    // frame chunks sized as a tracking call's, never below two frames (plan_blocks_stack: a pair's reference and image lie
    // in one stack); a frame chunk's upload, then every pair's chain (blocks_pair) in stream order: the next upload
    // overwrites the stack behind this chunk's last reader, and the host waits for none of them
    for (const StackChunk& S : plan_blocks_stack(n_frames, track_chunk_frames(c, rows, cols, chans), mode)) {
        px.assign(1, frames[S.carried]);
        px.insert(px.end(), frames + S.f0, frames + S.f0 + S.nf);
        adopt_image(c, (S.nf + 1) * rows, cols, chans, dtype);
        MTMC(upload_image_stack(c, c->slot[c->cur], px.data(), S.nf + 1, row_stride_bytes, rows, cols, chans, dtype, c->stream));
        for (int i = 0; i < S.nf; ++i) {
            const size_t p = (size_t)(S.p0 + i);
            const BlockSink sink{ens ? nullptr : c->blk_keys.as<unsigned long long>() + p * n,
                                 nbhd ? c->blk_nbhd.as<float>() + 9 * p * n : nullptr, ens ? (int)side : 0, p == 0 ? 1 : 0};
            MTMC(blocks_pair(c, P, ctx_block_tables(c), rows, chans, dtype, method, mode == MTM_BLOCKS_REF_FIRST ? 0 : i, i + 1,
                             !(gather_once && i > 0), sink));
        }
    }

    // the keys (and neighbourhoods), or the planes' sums, come back behind the call's single wait
    std::vector<unsigned long long> hkeys(ens ? 0 : np * n);
    std::vector<double> hacc(cells);
    MTMC(finish_block_call(c, {{ens ? hacc.data() : nullptr, c->blk_acc.p, sizeof(double) * cells},
                               {ens ? nullptr : hkeys.data(), c->blk_keys.p, sizeof(unsigned long long) * np * n},
                               {nbhd, c->blk_nbhd.p, sizeof(float) * 9 * np * n}}, ens ? n : np * n));
    if (ens) {
        // the mean of the pairs in float64, rounded to float32; NaN where the clipped box has no output
        const size_t sd = (size_t)side;
        const double pairs = (double)np;
        for (size_t k = 0; k < n; ++k) {
            const TrackUnit& u = P.units[k];
            const size_t ox = (size_t)P.clip[2 * k], oy = (size_t)P.clip[2 * k + 1];
            for (size_t cy = 0; cy < sd; ++cy)
                for (size_t cx = 0; cx < sd; ++cx) {
                    const size_t i = (k * sd + cy) * sd + cx;
                    const bool in = cy >= oy && cy - oy < (size_t)u.oh && cx >= ox && cx - ox < (size_t)u.ow;
                    planes[i] = in ? (float)(hacc[i] / pairs) : NAN;
                }
        }
    } else {
        for (size_t p = 0; p < np; ++p) decode_block_keys(P, blocks, hkeys.data() + p * n, method, out_hits + p * n);
    }
    return MTM_OK;
}

}  // extern "C"
