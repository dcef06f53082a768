// rpt_glare.hip.h — the opt-in glare stage of the splat passes (rpt_set_glare; not in the reference): a point-spread
// function of up to three separable Gaussian layers, convolved in exact integers over the passes' fixed-point accumulator between a
// pass's splat and its resolve.  Kernel 1170 convolves along the rows into one scratch plane per layer; kernel 1171 convolves those
// along the columns, adds the core, tonemaps as 1121 and 1131 do and leaves the accumulator all zero.  Included by rpt_api.hip behind
// rpt_particles.hip.h, whose helpers (hable1, to_u8, cl_min, RPT_STARS_ONE) it uses as they are.  tests/native/glare_oracle.c restates
// rules G2-G6 in C; the taps of rule G1 are host code (rpt_glare_taps).
#pragma once

#include "rpt_particles.hip.h"

#pragma clang fp contract(off)

namespace rptd {

#define RPT_GLARE_RADIUS 32                     /* the largest radius of a layer: min(32, ceil(3 sigma)) */
#define RPT_GLARE_SEGMENT 256                   /* 1170: pixels of one row per workgroup */
#define RPT_GLARE_TILE 16                       /* 1171: a workgroup's tile is 16 x 16 pixels */
#define RPT_GLARE_SOURCE_MAX (1ull << 44)       /* rule G2 */
#ifndef RPT_GLARE_SKIP
#define RPT_GLARE_SKIP 1                        /* 0 (tools/glare_cost.py's second library): no wave and no tile skips its arithmetic; the same bytes */
#endif

struct GlareArgs {
    unsigned long long *acc;            // [height * width * 3] the pass's sums; 1170 reads them, 1171 reads them again and zeroes them
    unsigned long long *planes;         // [layers][height * width * 3] h_k, written by 1170 (every word of the frame), read by 1171
    const rpt_event *events;            // the star pass: [height][width] records, a hit pixel is no source (rule G2); null in the other passes
    rpt_pixel *out16;                   // the framebuffer: only the dword at byte 8 of a pixel is read and written
    unsigned long long *counts;         // [1]: pixels whose bytes changed
    unsigned long long pixels;          // width * height
    int width, height;
    int wrap;                           // the splat's: a full-circle panorama, columns are taken modulo the width
    int layers;                         // 1 .. RPT_GLARE_LAYERS_MAX
    float hable_wp[3];
    unsigned int weight[1 + RPT_GLARE_LAYERS_MAX];      // w_0 (the core), w_1 .. (rule G0); they sum to 65536
    int radius[RPT_GLARE_LAYERS_MAX];
    unsigned int taps[RPT_GLARE_LAYERS_MAX][RPT_GLARE_RADIUS + 1];     // t_k[|j|] (rule G1); t_k[0] + 2 sum t_k[j > 0] = 65536
};

// sum += t * a in 64 bits on the halves of a: the low half is one 32 x 32 + 64 multiply-add, the high half (a <= 2^45, t <= 2^16)
// stays in 32 bits
RPT_DEV void glare_mad(unsigned long long &lo, unsigned int &hi, unsigned int t, unsigned long long a) {
    lo += (unsigned long long)t * (unsigned long long)(unsigned int)a;
    hi += t * (unsigned int)(a >> 32);
}

// Rule G2 for pixel p (p < a.pixels): the three sums clamped, zero where the star pass's record is a hit.  The record is read only
// where a sum is non-zero, as 1121 reads it.
RPT_DEV void glare_source(const GlareArgs &a, unsigned long long p, unsigned long long s[3]) {
    const unsigned long long *word = a.acc + p * 3ull;
    for (int c = 0; c < 3; c++) s[c] = word[c] < RPT_GLARE_SOURCE_MAX ? word[c] : RPT_GLARE_SOURCE_MAX;
    if ((s[0] | s[1] | s[2]) != 0ull && a.events) {
        const int object = *reinterpret_cast<const int *>(a.events + p);
        if (object >= 0) s[0] = s[1] = s[2] = 0ull;
    }
}

// 1170: rule G3.  grid (segments of a row, rows), 256 lanes: a workgroup stages its 256 pixels and 32 more on each side, per channel,
// in LDS (7.5 KB) — zero outside the frame, or the column modulo the width with `wrap` — and every lane writes its pixel's h_k for every
// layer.  A wave whose 64 + 64 staged columns are all zero, which is nearly every wave, writes zeros and multiplies nothing.  Every
// column is bounded by the width before it indexes the accumulator or the records, and only lanes with x < width write the planes.  The
// accumulator is left as it is: a segment's halo is its neighbours' own.
__global__ __launch_bounds__(RPT_GLARE_SEGMENT) void rpt_glare_rows_kernel(const GlareArgs a) {
    constexpr int kStaged = RPT_GLARE_SEGMENT + 2 * RPT_GLARE_RADIUS;
    __shared__ unsigned long long staged[3][kStaged];
    const int t = (int)threadIdx.x;
    const int y = (int)blockIdx.y;
    const int x0 = (int)blockIdx.x * RPT_GLARE_SEGMENT;
    if (y >= a.height || x0 >= a.width) return;          // (block-uniform; the host's grid has no such block)
    const unsigned long long row = (unsigned long long)y * (unsigned long long)a.width;
    for (int i = t; i < kStaged; i += RPT_GLARE_SEGMENT) {
        int x = x0 - RPT_GLARE_RADIUS + i;
        if (a.wrap) {
            x %= a.width;
            if (x < 0) x += a.width;
        }
        unsigned long long s[3] = {0ull, 0ull, 0ull};
        if (x >= 0 && x < a.width) glare_source(a, row + (unsigned long long)x, s);
        for (int c = 0; c < 3; c++) staged[c][i] = s[c];
    }
    __syncthreads();
    const int wave0 = t & ~63, l = t & 63;               // the wave's pixels are staged[.][wave0 + 32 .. wave0 + 96)
    unsigned long long any = 0ull;
    for (int c = 0; c < 3; c++) any |= staged[c][wave0 + l] | staged[c][wave0 + 64 + l];
    const bool lit = !RPT_GLARE_SKIP || __ballot(any != 0ull) != 0ull;      // wave-uniform
    const int x = x0 + t;
    if (x >= a.width) return;
    unsigned long long *out = a.planes + (row + (unsigned long long)x) * 3ull;
    const unsigned long long plane = a.pixels * 3ull;
    for (int k = 0; k < a.layers; k++, out += plane) {
        unsigned long long h[3] = {0ull, 0ull, 0ull};
        if (lit) {
            const int R = a.radius[k] < RPT_GLARE_RADIUS ? a.radius[k] : RPT_GLARE_RADIUS;
            for (int c = 0; c < 3; c++) {
                const unsigned long long *centre = &staged[c][t + RPT_GLARE_RADIUS];
                unsigned long long lo = 0ull;
                unsigned int hi = 0u;
                glare_mad(lo, hi, a.taps[k][0], centre[0]);
                for (int j = 1; j <= R; j++) glare_mad(lo, hi, a.taps[k][j], centre[-j] + centre[j]);
                h[c] = (lo + ((unsigned long long)hi << 32)) >> 16;
            }
        }
        out[0] = h[0];
        out[1] = h[1];
        out[2] = h[2];
    }
}

// 1171: rules G4-G6 for a tile of 16 x 16 pixels.  Per layer and channel the tile's columns of h_k, rows y0 - R .. y0 + 15 + R, are
// staged in LDS (at most 80 x 16 words, 10 KB; a row outside the frame is zero), and where any staged word is non-zero — block-uniform,
// and nearly nowhere — every lane sums its column's taps.  Then the pixel's own source again (rule G2) for the core, its accumulator
// words zeroed where they are not, rule G5, and where an S is non-zero the tonemap and the saturating add of 1121 and 1131, on hit and
// miss pixels alike.  Changed pixels are counted as 1121 counts them.  Every row and column is bounded by the frame before it indexes a
// plane, the accumulator, the records or the framebuffer.
__global__ __launch_bounds__(RPT_GLARE_TILE * RPT_GLARE_TILE) void rpt_glare_columns_kernel(const GlareArgs a) {
    constexpr int kLanes = RPT_GLARE_TILE * RPT_GLARE_TILE;
    constexpr int kRows = RPT_GLARE_TILE + 2 * RPT_GLARE_RADIUS;
    __shared__ unsigned long long staged[kRows * RPT_GLARE_TILE];
    __shared__ unsigned int block_changed;
    const int t = (int)threadIdx.x;
    const int lx = t & (RPT_GLARE_TILE - 1), ly = t / RPT_GLARE_TILE;
    const int x0 = (int)blockIdx.x * RPT_GLARE_TILE, y0 = (int)blockIdx.y * RPT_GLARE_TILE;
    const int x = x0 + lx, y = y0 + ly;
    const bool inside = x < a.width && y < a.height;
    if (t == 0) block_changed = 0u;
    unsigned long long S[3] = {0ull, 0ull, 0ull};
    const unsigned long long plane = a.pixels * 3ull;
    for (int k = 0; k < a.layers; k++) {
        const int R = a.radius[k] < RPT_GLARE_RADIUS ? a.radius[k] : RPT_GLARE_RADIUS;
        const int rows = RPT_GLARE_TILE + 2 * R;
        const unsigned long long *h = a.planes + (unsigned long long)k * plane;
        for (int c = 0; c < 3; c++) {
            __syncthreads();                             // (the last round's reads are done)
            int some = 0;
            for (int i = t; i < rows * RPT_GLARE_TILE; i += kLanes) {
                const int yy = y0 - R + i / RPT_GLARE_TILE, xx = x0 + (i & (RPT_GLARE_TILE - 1));
                unsigned long long v = 0ull;
                if (yy >= 0 && yy < a.height && xx < a.width) v = h[((unsigned long long)yy * (unsigned long long)a.width + (unsigned long long)xx) * 3ull + (unsigned long long)c];
                staged[i] = v;
                some |= v != 0ull;
            }
            const int lit = __syncthreads_or(some);      // block-uniform
            if (RPT_GLARE_SKIP && !lit) continue;
            const unsigned long long *centre = &staged[(ly + R) * RPT_GLARE_TILE + lx];
            unsigned long long lo = 0ull;
            unsigned int hi = 0u;
            glare_mad(lo, hi, a.taps[k][0], centre[0]);
            for (int j = 1; j <= R; j++) glare_mad(lo, hi, a.taps[k][j], centre[-j * RPT_GLARE_TILE] + centre[j * RPT_GLARE_TILE]);
            const unsigned long long v = (lo + ((unsigned long long)hi << 32)) >> 16;
            unsigned int top = 0u;
            glare_mad(S[c], top, a.weight[1 + k], v);
            S[c] += (unsigned long long)top << 32;
        }
    }
    bool changed = false;
    if (inside) {
        const unsigned long long p = (unsigned long long)y * (unsigned long long)a.width + (unsigned long long)x;
        unsigned long long *word = a.acc + p * 3ull;
        if ((word[0] | word[1] | word[2]) != 0ull) {
            unsigned long long s[3];
            glare_source(a, p, s);
            word[0] = 0ull;
            word[1] = 0ull;
            word[2] = 0ull;
            for (int c = 0; c < 3; c++) {
                unsigned int top = 0u;
                glare_mad(S[c], top, a.weight[0], s[c]);
                S[c] += (unsigned long long)top << 32;
            }
        }
        for (int c = 0; c < 3; c++) S[c] >>= 16;
        if ((S[0] | S[1] | S[2]) != 0ull) {
            uint32_t *rgba = reinterpret_cast<uint32_t *>(a.out16 + p) + 2;
            const uint32_t before = *rgba;
            uint32_t now = before & 0xff000000u;
            for (int c = 0; c < 3; c++) {
                const float sum = (float)S[c] * (1.0f / RPT_STARS_ONE);
                const uint32_t add = to_u8(cl_min(hable1(sum) / a.hable_wp[c], 1.0f));
                const uint32_t byte = ((before >> (8 * c)) & 255u) + add;
                now |= (byte > 255u ? 255u : byte) << (8 * c);
            }
            changed = now != before;
            if (changed) *rgba = now;
        }
    }
    const unsigned long long set = __ballot(changed);
    __syncthreads();                                     // (block_changed is zero, and every lane is past its last round)
    if ((t & 63) == 0 && set) atomicAdd(&block_changed, (unsigned int)__popcll(set));
    __syncthreads();
    if (t == 0 && block_changed) atomicAdd(a.counts + 1, (unsigned long long)block_changed);
}

}  // namespace rptd
