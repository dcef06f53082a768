// rpt_tile_bitmap.hpp — the per-object TILE BITMAP of a mesh: one bit per 8x8-pixel tile of the frame, 0 = "no primary ray of this
// tile can report a hit of this mesh".  The wave's object mask (rpt_kernels.hip.h: wave_object_mask) keeps a mesh for every tile that
// touches the proven rectangle or octagon around its ROOT box; a silhouette like the bunny's fills well under that octagon, and every
// lane of a tile between silhouette and octagon passes the root's slab test, walks the octree front to back through leaves whose
// triangles it misses — the longest kind of walk, it cannot stop at a first hit — and reports a miss.  The bitmap takes those tiles
// out: the octree is cut at a fixed depth into at most MAX_BOXES sub-trees that hold triangles, each sub-tree gets the box of the
// VERTICES of the triangles its leaf lists name, each such box a proven screen region of its own, and a tile whose grown square touches
// none of these regions has its bit cleared.  Host code only; nothing here is sampled or measured.
//
// SOUNDNESS.  Let a primary ray of pixel q report a hit of the mesh in the kernel's float arithmetic.
//  (a) The walk reports nothing but a Moeller-Trumbore hit of a triangle T that some LEAF list names (octree_walk, rpt_kernels.hip.h;
//      opencl_kernel.cl:106-126, 200-308); that leaf lies in exactly one sub-tree S of the cut (a leaf above the cut depth is a sub-tree
//      of its own), so all three vertices of T lie in S's vertex box V — by construction, whatever the node boxes are: a listed
//      triangle may reach beyond its leaf, which is why the node box is not used.
//  (b) rpt_kernels.hip.h, mesh_segment_apart (i): with o the float origin the kernel reads (DObj.ox/oy/oz), g the float direction and
//      dist >= 0 the accepted float distance, the float point Q = o + g dist lies within
//          16.2 K tau + u (tau + 2.1 dist + 2.1 max(|e1|, |e2|))  +  u max(|e1|, |e2|)      of a point of T,
//      K = the largest |e1| |e2| of the mesh's triangles, tau = |o - A| <= tau_max := |o| + (the distance from o to V's far corner)
//      (A is a vertex of T, hence a point of V; the |o| on top is slack).  With dist <= tau_max + that bound and L the longest edge this
//      is at most  m := (16.2 K + 3.2u) tau_max 1.001 + 4u L, and the EXACT point o + g dist of the exact forward ray along the float
//      direction differs from Q by one rounding per component: at most 2.1u (|o_k| + tau_max + m).  The rule 16.2 K + 3.2u <= 0.25
//      (the one mesh_segment_apart already uses, DObj::mslope >= 0) decides whether the bound is of any use: bunny.obj has 0.0046,
//      pear.obj 3.1 and gets no bitmap.
//  (c) Hence the exact forward ray from o along the float direction meets  V grown by  m + 8u (|o|_inf + tau_max)  per axis — a box,
//      a convex set, handed to the certificate as `root_bounds` (cert::setup grows it once more by its own 4u term, which only
//      enlarges it).  That is the premise of rpt_bounds_certify.hpp, section 2 ("float hit => the exact forward ray from o along the
//      float direction meets the convex set B'"), and section 3 proves for ANY such box and any claimed region: with twice the
//      direction's error budget no pixel of the frame outside the claimed region can make that statement true.  So q lies in the proven
//      region of S's box.  A box whose region cannot be proven would get the full plane and set every bit; build() then returns no
//      bitmap at all (nothing would be gained, and the kernel's load is saved): ONE sub-tree box the camera is inside of or too near
//      to — a fly-by, a close-up — costs the mesh its whole bitmap for that view, and the kernel keeps the root box's mask.
//  (d) wave_object_mask's skirt: pixel (x, y) of tile (tx, ty) looks through a plane point inside the tile's square grown by a pixel
//      and a half (rpt_kernels.hip.h: the float chains of the pixel and of the tile's edges are 3u and 4u aspect off, against a skirt
//      of 1.5 aspect / W).  The squares are evaluated in DOUBLE here (error 1e-16 instead of 4u: the pixel's own 3u aspect is all that
//      is left to cover, and 2^20 pixels a side leave the skirt 1.5 / (3u 2^20) = 8 times larger), with the lens factor s applied to
//      all four sides as wave_object_mask_lens does.  q's plane point lies in its tile's grown square and in the region of (c), so
//      that tile's square meets the region and its bit is set.                                                              q.e.d.
// The bitmap is a function of the object's 320 bytes, the interval, the mesh's boxes, the frame's size and the lens — nothing else.
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/rpt_layout.h"
#include "rpt_bounds_certify.hpp"

namespace rptb {
namespace tiles {

constexpr int MAX_BOXES = 64;          // sub-trees with triangles per mesh (a cut at depth 2 never has more)

// The cut of the octree under `root`: the deepest level at which at most `max_boxes` sub-trees hold triangles, and for each of them
// the box of the vertices of every triangle its leaf lists name (six floats: min.xyz, max.xyz).  false: an index out of range, a
// child loop, a non-finite vertex, or more than `max_boxes` sub-trees already at depth 1 — the mesh gets no boxes.
inline bool subtree_boxes(const rpt_scene_desc &s, int root, int max_boxes, std::vector<float> &boxes, int *depth_out = nullptr) {
    boxes.clear();
    if (root < 0 || (size_t)root >= s.octree_count || max_boxes < 1) return false;
    const size_t n_tris = s.triangle_words / 9;
    // level by level; a leaf above the cut stays in the frontier as it is
    std::vector<int> frontier{root}, next;
    std::vector<float> best;
    int best_depth = -1;
    size_t visited = 1;
    for (int depth = 0; depth <= 8; depth++) {
        // the boxes of this frontier
        std::vector<float> level;
        bool ok = true;
        for (int node : frontier) {
            float b[6] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY};
            bool any = false;
            std::vector<int> stack{node};
            size_t steps = 0;
            while (!stack.empty() && ok) {
                const int k = stack.back();
                stack.pop_back();
                if (++steps > s.octree_count) { ok = false; break; }        // (a child loop)
                const rpt_octree &o = s.octrees[k];
                if (o.children[0] != -1) {
                    for (int c = 0; c < 8; c++) {
                        if (o.children[c] < 0 || (size_t)o.children[c] >= s.octree_count) { ok = false; break; }
                        stack.push_back(o.children[c]);
                    }
                    continue;
                }
                if (o.trisCount < 0 || o.trisIndex < 0 || (size_t)o.trisIndex + (size_t)o.trisCount > s.octree_tri_count) { ok = false; break; }
                for (int t0 = o.trisIndex; t0 < o.trisIndex + o.trisCount && ok; t0++) {
                    const int t = s.octreeTris[t0];
                    if (t < 0 || (size_t)t >= n_tris) { ok = false; break; }
                    for (int c = 0; c < 3; c++) {
                        const uint32_t w = s.triangles[9 * (size_t)t + 3 * c];
                        if (w >= s.vertex_count) { ok = false; break; }
                        const rpt_float3 &v = s.vertices[w];
                        if (!std::isfinite(v.x) || !std::isfinite(v.y) || !std::isfinite(v.z)) { ok = false; break; }
                        b[0] = std::fmin(b[0], v.x); b[1] = std::fmin(b[1], v.y); b[2] = std::fmin(b[2], v.z);
                        b[3] = std::fmax(b[3], v.x); b[4] = std::fmax(b[4], v.y); b[5] = std::fmax(b[5], v.z);
                        any = true;
                    }
                }
            }
            if (!ok) break;
            if (any) level.insert(level.end(), b, b + 6);
        }
        if (!ok) return false;
        if (level.size() > (size_t)max_boxes * 6) break;
        best.swap(level);
        best_depth = depth;
        // one level down
        next.clear();
        bool split = false;
        for (int node : frontier) {
            const rpt_octree &o = s.octrees[node];
            if (o.children[0] == -1) { next.push_back(node); continue; }
            for (int c = 0; c < 8; c++) {
                if (o.children[c] < 0 || (size_t)o.children[c] >= s.octree_count) return false;
                next.push_back(o.children[c]);
            }
            split = true;
        }
        visited += next.size();
        if (!split || visited > 8 * s.octree_count + 8) break;
        frontier.swap(next);
    }
    if (best_depth < 0) return false;
    boxes.swap(best);
    if (depth_out) *depth_out = best_depth;
    return true;
}

struct Frame {
    int width, height;
    float lens_scale;       // 1.0f: the reference's lens
    bool diagonals;         // the frame lies inside the diagonal slabs' window (what KernelArgs::diagonals asks of the frame)
};

inline size_t bitmap_words(int width, int height) { return ((size_t)((width + 7) / 8) * (size_t)((height + 7) / 8) + 31) / 32; }

struct Stats { int boxes, proven, tiles_set, tiles; };

// One sub-tree box grown by the margin of (b) and (c) above, rounded outward to floats.  false: nothing finite came out.
inline bool grown_box(const float o[3], const float box[6], double slope, double L, float out[6]) {
    const double U = cert::U24;
    double o2 = 0.0, far2 = 0.0, oinf = 0.0;
    for (int k = 0; k < 3; k++) {
        if (!std::isfinite(box[k]) || !std::isfinite(box[k + 3]) || !(box[k] <= box[k + 3]) || !std::isfinite(o[k])) return false;
        o2 += (double)o[k] * o[k];
        const double d = std::max(std::fabs((double)o[k] - box[k]), std::fabs((double)o[k] - box[k + 3]));
        far2 += d * d;
        oinf = std::max(oinf, std::fabs((double)o[k]));
    }
    const double tau_max = (std::sqrt(o2) + std::sqrt(far2)) * (1.0 + 1.0e-12);
    const double m = slope * tau_max * 1.001 + 4.0 * U * L + 1.0e-30;
    const double g = m + 8.0 * U * (oinf + tau_max + m);
    for (int k = 0; k < 3; k++) {
        out[k] = std::nextafter((float)((double)box[k] - g), -INFINITY);
        out[k + 3] = std::nextafter((float)((double)box[k + 3] + g), INFINITY);
        if (!std::isfinite(out[k]) || !std::isfinite(out[k + 3])) return false;
    }
    return true;
}

// The bitmap of mesh object `ob` (`bits`: bitmap_words() dwords, bit ty * tiles_x + tx of the frame's 8x8 tiles).  `boxes`: n_boxes
// sub-tree boxes of its mesh; `slope` = 16.2 K + 3.2u and `L` of that mesh (the caller has checked slope <= 0.25).
// false: no bitmap — a box that is not a box, or one whose region could not be proven (every bit would be set: nothing to gain).
inline bool build(const rpt_object &ob, int interval, const float *boxes, int n_boxes, double slope, double L, const Frame &f,
                  uint32_t *bits, Stats *stats = nullptr) {
    if (stats) *stats = Stats{n_boxes, 0, 0, 0};
    if (ob.type != RPT_MESH || n_boxes < 1 || !boxes || f.width < 1 || f.height < 1 || !(slope >= 0.0) || !(slope <= 0.25) || !std::isfinite(L)) return false;
    if (!(f.lens_scale > 0.0f) || !(f.lens_scale <= 1.0f)) return false;
    const int tx_n = (f.width + 7) / 8, ty_n = (f.height + 7) / 8;
    const size_t words = bitmap_words(f.width, f.height);
    for (size_t k = 0; k < words; k++) bits[k] = 0u;
    // the tiles' grown squares on the image plane (d) — in double
    const double W = f.width, H = f.height, aspect = (double)((float)f.width / (float)f.height), s = f.lens_scale;
    std::vector<double> tu0((size_t)tx_n), tu1((size_t)tx_n), tv0((size_t)ty_n), tv1((size_t)ty_n);
    for (int tx = 0; tx < tx_n; tx++) {
        tu0[(size_t)tx] = s * (((8.0 * tx - 1.5) / W - 0.5) * aspect);
        tu1[(size_t)tx] = s * (((8.0 * tx + 8.5) / W - 0.5) * aspect);
    }
    for (int ty = 0; ty < ty_n; ty++) {
        tv0[(size_t)ty] = s * ((8.0 * ty - 1.5) / H - 0.5);
        tv1[(size_t)ty] = s * ((8.0 * ty + 8.5) / H - 0.5);
    }
    float o[3];
    cert::kernel_origin(ob, o);
    int proven = 0;
    for (int b = 0; b < n_boxes; b++) {
        float g[6];
        if (!grown_box(o, boxes + 6 * b, slope, L, g)) return false;
        const Rect r = certified_object_rect(ob, interval, g);          // proposed, then PROVEN or the full plane
        if (r.u0 <= -3.0e38f && r.v0 <= -3.0e38f && r.u1 >= 3.0e38f && r.v1 >= 3.0e38f && !has_diagonals(r)) return false;
        proven++;
        if (!(r.u0 <= r.u1) || !(r.v0 <= r.v1)) {
            if (r.u0 != r.u0 || r.u1 != r.u1 || r.v0 != r.v0 || r.v1 != r.v1) return false;      // (a NaN keeps its object in the kernel: no bitmap)
            continue;                                                                            // proven invisible: sets nothing
        }
        const bool diag = f.diagonals && has_diagonals(r);
        for (int ty = 0; ty < ty_n; ty++) {
            const double v0 = tv0[(size_t)ty], v1 = tv1[(size_t)ty];
            if ((double)r.v1 < v0 || (double)r.v0 > v1) continue;
            for (int tx = 0; tx < tx_n; tx++) {
                const double u0 = tu0[(size_t)tx], u1 = tu1[(size_t)tx];
                bool outside = (double)r.u1 < u0 || (double)r.u0 > u1;
                if (diag) outside = outside || (double)r.p_hi < u0 + v0 || (double)r.p_lo > u1 + v1 || (double)r.m_hi < u0 - v1 || (double)r.m_lo > u1 - v0;
                if (outside) continue;
                const size_t t = (size_t)ty * tx_n + tx;
                bits[t >> 5] |= 1u << (t & 31);
            }
        }
    }
    if (stats) {
        int set = 0;
        for (size_t k = 0; k < words; k++) set += __builtin_popcount(bits[k]);
        *stats = Stats{n_boxes, proven, set, tx_n * ty_n};
    }
    return true;
}

}  // namespace tiles
}  // namespace rptb
