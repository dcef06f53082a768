// rpt_stars_host.hpp — the part of the star-field pass (rpt_set_stars / rpt_render_stars) that needs no device: the
// catalogue's validation, the normalisation of its directions, and the sky-to-camera matrix G.  Plain C++17, no HIP:
// rpt_api.hip includes it, and tests/native/stars_host_main.cpp compiles it alone (under the address and undefined-behaviour sanitizers).
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/rpt.h"

namespace rpts {

constexpr int kMaxStars = 1 << 22;      // 2^22 stars x 2^40 per tap cannot overflow a 64-bit accumulator

// "" = the catalogue is acceptable; otherwise what rpt_set_stars refuses it for (entry index and field)
inline std::string catalogue_fault(const rpt_star *stars, int count) {
    if (count < 0 || count > kMaxStars) return "count is 0 .. 2^22 (4194304)";
    if (count > 0 && !stars) return "a null catalogue with count > 0";
    for (int i = 0; i < count; i++) {
        const rpt_star &s = stars[i];
        const std::string which = "entry " + std::to_string(i) + ": ";
        for (int k = 0; k < 3; k++) {
            if (!std::isfinite(s.dir[k]) || !std::isfinite(s.rgb[k])) return which + "every component of dir and rgb must be finite";
            if (s.rgb[k] < 0.0f) return which + "a colour channel is negative";
        }
        if (s.dir[0] == 0.0f && s.dir[1] == 0.0f && s.dir[2] == 0.0f) return which + "dir has zero length";
    }
    return "";
}

// dir / |dir| with the length formed in double (a float's square cannot underflow or overflow there), each quotient rounded to float once
inline void normalise_direction(const float in[3], float out[3]) {
    const double x = in[0], y = in[1], z = in[2];
    const double l = std::sqrt(x * x + y * y + z * z);
    out[0] = (float)(x / l);
    out[1] = (float)(y / l);
    out[2] = (float)(z / l);
}

// The catalogue as the device reads it, in the caller's order: directions normalised, colours copied, padding zero.  `stars` has passed
// catalogue_fault.  (A spatial order — Morton keys over the faces of a cube — was built and measured, and did not pay: DESIGN.md §19.)
inline void prepare_catalogue(const rpt_star *stars, int count, rpt_star *out) {
    for (int i = 0; i < count; i++) {
        rpt_star s;
        std::memset(&s, 0, sizeof s);
        normalise_direction(stars[i].dir, s.dir);
        for (int k = 0; k < 3; k++) s.rgb[k] = stars[i].rgb[k];
        out[i] = s;
    }
}

// a^-1 for an n x n matrix (n <= 4, row-major) by Gauss-Jordan elimination with partial pivoting, in double.  false: singular — a pivot
// no larger than 1e-12 times the matrix's largest entry (an all-zero matrix included) — or a non-finite entry.
inline bool invert(const double *a, int n, double *inv) {
    double m[4][8];
    double scale = 0.0;
    for (int r = 0; r < n; r++)
        for (int c = 0; c < n; c++) {
            if (!std::isfinite(a[r * n + c])) return false;
            m[r][c] = a[r * n + c];
            m[r][n + c] = r == c ? 1.0 : 0.0;
            scale = std::max(scale, std::fabs(a[r * n + c]));
        }
    for (int col = 0; col < n; col++) {
        int p = col;
        for (int r = col + 1; r < n; r++)
            if (std::fabs(m[r][col]) > std::fabs(m[p][col])) p = r;
        if (!(std::fabs(m[p][col]) > 1e-12 * scale)) return false;
        if (p != col)
            for (int c = 0; c < 2 * n; c++) std::swap(m[p][c], m[col][c]);
        const double d = m[col][col];
        for (int c = 0; c < 2 * n; c++) m[col][c] /= d;
        for (int r = 0; r < n; r++) {
            if (r == col) continue;
            const double f = m[r][col];
            if (f == 0.0) continue;
            for (int c = 0; c < 2 * n; c++) m[r][c] -= f * m[col][c];
        }
    }
    for (int r = 0; r < n; r++)
        for (int c = 0; c < n; c++) inv[r * n + c] = m[r][n + c];
    return true;
}

// G of DESIGN.md §19 rule 1 from E' (row-major, t first): with light delay on (interval != 0) the inverse of all of E'; with it off the
// sky lookup sees only E's spatial block, so G is that block's inverse under a first row and column of the identity.  Inverted in
// double, rounded to float once.  false: E' (or the block) cannot be inverted, or an entry of G is not a finite float.
inline bool sky_to_camera(const float e[16], int interval, float g[16]) {
    double a[16], inv[16];
    if (interval != 0) {
        for (int k = 0; k < 16; k++) a[k] = e[k];
        if (!invert(a, 4, inv)) return false;
        for (int k = 0; k < 16; k++) g[k] = (float)inv[k];
    } else {
        for (int r = 0; r < 3; r++)
            for (int c = 0; c < 3; c++) a[r * 3 + c] = e[(r + 1) * 4 + (c + 1)];
        if (!invert(a, 3, inv)) return false;
        for (int k = 0; k < 16; k++) g[k] = (k % 5 == 0) ? 1.0f : 0.0f;
        for (int r = 0; r < 3; r++)
            for (int c = 0; c < 3; c++) g[(r + 1) * 4 + (c + 1)] = (float)inv[r * 3 + c];
    }
    for (int k = 0; k < 16; k++)
        if (!std::isfinite(g[k])) return false;
    return true;
}

}  // namespace rpts
