// rpt_sky_split.hpp — host side of the sky split: the box of 8x8 tiles outside of which the wave's object mask
// (rpt_kernels.hip.h: wave_object_mask) is empty for every tile of a frame.  Plain C++, no HIP: rpt_api.hip's launch() calls it once
// per frame, tests/native/sky_split_main.cpp holds it against a float32 restatement of the device's test.
//
// The device keeps object i for the tile with corner (x0, y0) unless
//     r.u1 < tu0  or  r.u0 > tu1  or  r.v1 < tv0  or  r.v0 > tv1        (a NaN compares false: it keeps the object)
// with tu0 = fl(((x0 - 1.5) / W - 1/2) aspect), tu1 = fl(((x0 + 8.5) / W - 1/2) aspect), tv0 / tv1 the same in y with H and aspect 1.
// In exact arithmetic, with P(c) = (c / aspect + 1/2) W the pixel coordinate of a plane coordinate c, column t = x0 / 8 is kept iff
//     8 t + 8.5 >= P(u0)  and  8 t - 1.5 <= P(u1).
// Of the two ways to be conservative against the device's float rounding — evaluating its float expressions tile by tile, or growing the
// exact answer by a whole tile — this takes the second: the range of kept columns is found from two divisions per object and side (the
// first costs a search over the columns, per object and frame, for the same box give or take a ring of tiles), and the margin is easy to
// state.  The device's tu0 / tu1 are off their exact values by at most 4u aspect on the plane, u = 2^-24 (the multiply by the rounded
// 1 / W, the subtraction, the multiply by aspect: rpt_kernels.hip.h counts them), i.e. by 4u W <= 0.25 pixel while W <= 2^20, which launch() enforces before it
// culls at all; the arithmetic here is double on the same float inputs (errors of 1e-10 pixel).  The range below starts a whole tile
// (8 pixels) before the first column the exact test keeps, and ends a whole tile behind the last: no rounding of a quarter pixel moves
// a kept tile out of it.  The diagonal slabs only ever drop an object from a tile, so they are ignored.
// An object whose rectangle is the full plane (an unproven bound; rptb::full_rect) or holds a NaN yields the whole axis, an empty
// rectangle (u0 > u1: behind the camera) nothing.
#pragma once
#include <cmath>

#include "rpt_screen_bounds.hpp"

namespace rpts {

// [lo, hi) of the `tiles` 8-pixel tiles along one axis that may keep an object whose plane range is [c0, c1]; `to_pixels` = W / aspect (or H)
inline void kept_tiles(float c0, float c1, double to_pixels, double size, int tiles, int &lo, int &hi) {
    const double p0 = (double)c0 * to_pixels + 0.5 * size, p1 = (double)c1 * to_pixels + 0.5 * size;
    lo = 0;
    hi = tiles;
    if (p0 > 8.5) lo = p0 >= 8.0 * tiles + 16.5 ? tiles : (int)std::floor((p0 - 8.5) / 8.0) - 1;      // (a NaN: the comparison fails, lo stays 0)
    if (p1 < 8.0 * tiles) hi = p1 <= -17.5 ? 0 : (int)std::floor((p1 + 1.5) / 8.0) + 2;
    if (lo < 0) lo = 0;
    if (hi > tiles) hi = tiles;
}

// The box [box[0], box[2]) x [box[1], box[3]) of tiles that holds every tile for which wave_object_mask is not 0, for the first
// min(count, 64) rectangles of a width x height frame.  false: no object keeps any tile (the box is left {0, 0, 0, 0}).
inline bool object_box(const rptb::Rect *rects, int count, int width, int height, int box[4]) {
    const int tiles_x = (width + 7) / 8, tiles_y = (height + 7) / 8;
    const double aspect = (double)((float)width / (float)height);      // KernelArgs::aspect, the float the device multiplies by
    int x0 = tiles_x, y0 = tiles_y, x1 = 0, y1 = 0;
    for (int i = 0; i < count && i < 64; i++) {
        int lx, hx, ly, hy;
        kept_tiles(rects[i].u0, rects[i].u1, (double)width / aspect, (double)width, tiles_x, lx, hx);
        kept_tiles(rects[i].v0, rects[i].v1, (double)height, (double)height, tiles_y, ly, hy);
        if (lx >= hx || ly >= hy) continue;
        if (lx < x0) x0 = lx;
        if (hx > x1) x1 = hx;
        if (ly < y0) y0 = ly;
        if (hy > y1) y1 = hy;
    }
    const bool any = x0 < x1 && y0 < y1;
    box[0] = any ? x0 : 0; box[1] = any ? y0 : 0; box[2] = any ? x1 : 0; box[3] = any ? y1 : 0;
    return any;
}

}  // namespace rpts
