// Where a block's search box goes when a displacement is predicted for it (mtm_match_blocks_at, mtm_match_blocks_passes;
// DESIGN 5.6.2), as inline functions for the host (plan_block_passes' callers, mtm_debug_plan_blocks_passes: mtm_host.cpp)
// and the device (blocks_unit_kernel, mtm_k_blocks.hip.h): a single source for the nearest-block rule and for the moved,
// clamped and clipped box, so that the boxes a test computes on the host are the boxes the kernels search.  Integers only.
#pragma once
#include <cstdint>

#include "../../include/mtm_hip.h"
#include "mtm_templ_stats.h"       // MTM_HOST_DEVICE

namespace mtm {

// One pass's regular grid of blocks (MTM.blocks.grid): bw x bh blocks at stride (sx, sy), nx columns and ny rows of them,
// block (iy, ix) - index iy nx + ix - at (ix sx, iy sy).
struct BlockGrid {
    int bw, bh, sx, sy, nx, ny;
};

MTM_HOST_DEVICE inline BlockGrid block_grid_of(const mtm_block_pass& p, int rows, int cols) {
    BlockGrid g{p.bw, p.bh, p.sx, p.sy, 0, 0};
    if (p.bw >= 1 && p.bh >= 1 && p.sx >= 1 && p.sy >= 1 && cols >= p.bw && rows >= p.bh) {
        g.nx = (cols - p.bw) / p.sx + 1;
        g.ny = (rows - p.bh) / p.sy + 1;
    }
    return g;
}

// Along one axis: the index of the coarse block (size wc, stride s, n >= 1 of them, block i at i s) whose centre is
// nearest to that of a fine block of size wf at x >= 0, decided on doubled centres 2 i s + wc and 2 x + wf; an exact tie
// goes to the higher index.  (MTM.blocks.predict_offsets states the same rule in numpy.)
MTM_HOST_DEVICE inline int blocks_nearest_inl(int n, int s, int wc, int x, int wf) {
    const long long num = 2ll * x + wf - wc + s;
    const long long i = (num > 0 ? num : 0) / (2ll * s);
    return (int)(i < n - 1 ? i : n - 1);
}

// The unit of block b moved by (dx, dy): the block's position is moved and clamped so that the block lies inside the
// rows x cols image, then its box is widened by `margin` on every side and clipped to the image
// (MTM.blocks.search_box_at).  A block inside the image gives a map of at least one output, whatever the offset.
struct BlockUnitBox {
    int y0, x0, oh, ow;
};
MTM_HOST_DEVICE inline BlockUnitBox blocks_unit_at_inl(const mtm_block& b, long long dx, long long dy, int margin, int rows,
                                                       int cols) {
    long long cx = (long long)b.x + dx, cy = (long long)b.y + dy;
    const long long mx = (long long)cols - b.w, my = (long long)rows - b.h;
    cx = cx < 0 ? 0 : (cx > mx ? mx : cx);
    cy = cy < 0 ? 0 : (cy > my ? my : cy);
    const long long x0 = cx - margin > 0 ? cx - margin : 0, y0 = cy - margin > 0 ? cy - margin : 0;
    const long long x1 = cx + b.w + margin < cols ? cx + b.w + margin : cols;
    const long long y1 = cy + b.h + margin < rows ? cy + b.h + margin : rows;
    return BlockUnitBox{(int)y0, (int)x0, (int)(y1 - y0 - b.h + 1), (int)(x1 - x0 - b.w + 1)};
}

// The moved and clamped position (cx, cy) blocks_unit_at_inl widens: MTM.blocks.moved_blocks' numbers.  The unit of the
// moved block starts at (x0, y0) = (max(cx - margin, 0), max(cy - margin, 0)), so output (y, x) of its map is cell
// (y + y0 - (cy - margin), x + x0 - (cx - margin)) of the block's (2 margin + 1)^2 plane of displacements around (cx, cy).
MTM_HOST_DEVICE inline void blocks_moved_at_inl(const mtm_block& b, long long dx, long long dy, int rows, int cols, int* cx,
                                                int* cy) {
    long long x = (long long)b.x + dx, y = (long long)b.y + dy;
    const long long mx = (long long)cols - b.w, my = (long long)rows - b.h;
    *cx = (int)(x < 0 ? 0 : (x > mx ? mx : x));
    *cy = (int)(y < 0 ? 0 : (y > my ? my : y));
}

// The displacement a pass predicts for block `b` of its own grid from the previous pass's records `prev` (image
// coordinates, one per block of grid `c` in grid order): that of the coarse block with the nearest centre.
MTM_HOST_DEVICE inline void blocks_predict_inl(const BlockGrid& c, const mtm_hit* prev, const mtm_block& b, long long* dx,
                                               long long* dy) {
    const int ix = blocks_nearest_inl(c.nx, c.sx, c.bw, b.x, b.w), iy = blocks_nearest_inl(c.ny, c.sy, c.bh, b.y, b.h);
    const mtm_hit& r = prev[(long long)iy * c.nx + ix];
    *dx = (long long)r.x - (long long)ix * c.sx;
    *dy = (long long)r.y - (long long)iy * c.sy;
}

}  // namespace mtm
