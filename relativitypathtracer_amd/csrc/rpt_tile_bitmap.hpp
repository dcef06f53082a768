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
//  (a') THE TRIANGLE STAGE (triangle_boxes): the same hit is a Moeller-Trumbore hit of a listed triangle T, and T's three vertices lie
//      in T's OWN vertex box V, the box triangle_boxes() made for T — every distinct triangle a leaf list under the root names has one.
//      Steps (b)-(d) speak of "a vertex box V that holds T's vertices" and of nothing else of the cut, so they apply to this V
//      unchanged: grown_box, certified_object_rect, the skirt.  (K and L stay the MESH's: maxima over all its triangles bound T's.)  The
//      stage is restricted as the sub-tree stage is: to meshes whose lists name only triangles inside the root's box and inside the
//      rule of (b).  Each stage alone is sound, so q's tile has its bit set in both and the AND of the two bitmaps is sound; the product
//      never sets a bit the sub-tree stage clears.  A triangle stage that yields nothing (more than the cap's triangles, a box that is
//      not a box, ONE triangle whose region cannot be proven) leaves the sub-tree stage alone; no sub-tree stage: no bitmap at all.
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
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/rpt_layout.h"
#include "rpt_bounds_certify.hpp"
#include "rpt_workers.hpp"

namespace rptb {
namespace tiles {

constexpr int MAX_BOXES = 64;          // sub-trees with triangles per mesh (a cut at depth 2 never has more)
// Distinct triangles per mesh the triangle stage takes on.  One box costs one proof and a rasterisation of a few tiles: 1.5 us on one
// core of the MI355X machine's host, from rpt_tile_bitmap_state's build times of bunny.obj at 3840x2160 with no helper threads —
// 7 580 us with the stage's 4 968 boxes, 127 us with the sub-tree stage's 47 alone (profiles/r20_tile_triangles_ab.txt).  The cap keeps
// a single-threaded build within 100 times today's 127 us: 8 192 boxes are 12.3 ms, 97 times.  Why 100: the build is paid once per still
// view and scene (contexts of one scene share it) and only after two identical rpt_set_objects calls, and 12 ms is the time of one
// frame on a 60-90 Hz display: the launch that builds it never stalls a still view for longer than one frame its viewer sees, with
// helper threads (four by default) for a quarter of that.  8 192 is the smallest power of two that holds bunny.obj's 4 968.  A denser
// mesh keeps the sub-tree stage's bitmap.
constexpr int MAX_TRIANGLES = 8192;

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

// The triangle stage's boxes: for every DISTINCT triangle the leaf lists under `root` name, in ascending order of its index, the box of
// its three vertices.  subtree_boxes' validations; false: an index out of range, a child loop, a non-finite vertex, or more than
// `max_triangles` triangles — the mesh gets no triangle stage.
inline bool triangle_boxes(const rpt_scene_desc &s, int root, int max_triangles, std::vector<float> &out) {
    out.clear();
    if (root < 0 || (size_t)root >= s.octree_count || max_triangles < 1) return false;
    const size_t n_tris = s.triangle_words / 9;
    std::vector<uint8_t> named(n_tris, 0);
    size_t distinct = 0, steps = 0;
    std::vector<int> stack{root};
    while (!stack.empty()) {
        const int k = stack.back();
        stack.pop_back();
        if (++steps > s.octree_count) return false;                         // (a child loop)
        const rpt_octree &o = s.octrees[k];
        if (o.children[0] != -1) {
            for (int c = 0; c < 8; c++) {
                if (o.children[c] < 0 || (size_t)o.children[c] >= s.octree_count) return false;
                stack.push_back(o.children[c]);
            }
            continue;
        }
        if (o.trisCount < 0 || o.trisIndex < 0 || (size_t)o.trisIndex + (size_t)o.trisCount > s.octree_tri_count) return false;
        for (int t0 = o.trisIndex; t0 < o.trisIndex + o.trisCount; t0++) {
            const int t = s.octreeTris[t0];
            if (t < 0 || (size_t)t >= n_tris) return false;
            if (named[(size_t)t]) continue;
            named[(size_t)t] = 1;
            if (++distinct > (size_t)max_triangles) return false;
        }
    }
    out.reserve(distinct * 6);
    for (size_t t = 0; t < n_tris; t++) {
        if (!named[t]) continue;
        float b[6] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY};
        for (int c = 0; c < 3; c++) {
            const uint32_t w = s.triangles[9 * t + 3 * c];
            if (w >= s.vertex_count) { out.clear(); return false; }
            const rpt_float3 &v = s.vertices[w];
            if (!std::isfinite(v.x) || !std::isfinite(v.y) || !std::isfinite(v.z)) { out.clear(); return false; }
            b[0] = std::fmin(b[0], v.x); b[1] = std::fmin(b[1], v.y); b[2] = std::fmin(b[2], v.z);
            b[3] = std::fmax(b[3], v.x); b[4] = std::fmax(b[4], v.y); b[5] = std::fmax(b[5], v.z);
        }
        out.insert(out.end(), b, b + 6);
    }
    return !out.empty();
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

// The tiles' grown squares on the image plane (d) — in double.  Every table ascends with its index (each operation that makes an entry is
// monotone in tx or ty, and rounding keeps order), which is what rasterise()'s ranges rest on.
struct Grid {
    int tx_n, ty_n;
    std::vector<double> tu0, tu1, tv0, tv1;
    explicit Grid(const Frame &f) : tx_n((f.width + 7) / 8), ty_n((f.height + 7) / 8), tu0((size_t)tx_n), tu1((size_t)tx_n), tv0((size_t)ty_n), tv1((size_t)ty_n) {
        const double W = f.width, H = f.height, aspect = (double)((float)f.width / (float)f.height), s = f.lens_scale;
        for (int tx = 0; tx < tx_n; tx++) {
            tu0[(size_t)tx] = s * (((8.0 * tx - 1.5) / W - 0.5) * aspect);
            tu1[(size_t)tx] = s * (((8.0 * tx + 8.5) / W - 0.5) * aspect);
        }
        for (int ty = 0; ty < ty_n; ty++) {
            tv0[(size_t)ty] = s * ((8.0 * ty - 1.5) / H - 0.5);
            tv1[(size_t)ty] = s * ((8.0 * ty + 8.5) / H - 0.5);
        }
    }
};

// [first, last) of the entries i with !(hi < lo_tab[i]) && !(lo > hi_tab[i]): both tables ascend, so "lo > hi_tab[i]" holds on a prefix
// and "hi < lo_tab[i]" on a suffix, and the same two comparisons a loop over every entry would make find the ends of what is left.
inline void tile_range(const std::vector<double> &lo_tab, const std::vector<double> &hi_tab, double lo, double hi, int &first, int &last) {
    first = (int)(std::partition_point(hi_tab.begin(), hi_tab.end(), [lo](double t1) { return lo > t1; }) - hi_tab.begin());
    last = (int)(std::partition_point(lo_tab.begin(), lo_tab.end(), [hi](double t0) { return !(hi < t0); }) - lo_tab.begin());
}

// Sets the bit of every tile whose grown square touches the region `r` (a rectangle with r.u0 <= r.u1, r.v0 <= r.v1; an octagon with
// `diag`): only the rows and columns the rectangle spans are visited — with 4 968 boxes and 480 columns a walk over every column of
// every overlapping row was most of the build — and inside them the tests are those of the full loop: the same bits.
inline void rasterise(const Rect &r, bool diag, const Grid &g, uint32_t *bits) {
    int ty0, ty1, tx0, tx1;
    tile_range(g.tv0, g.tv1, (double)r.v0, (double)r.v1, ty0, ty1);
    tile_range(g.tu0, g.tu1, (double)r.u0, (double)r.u1, tx0, tx1);
    for (int ty = ty0; ty < ty1; ty++) {
        const double v0 = g.tv0[(size_t)ty], v1 = g.tv1[(size_t)ty];
        for (int tx = tx0; tx < tx1; tx++) {
            if (diag) {
                const double u0 = g.tu0[(size_t)tx], u1 = g.tu1[(size_t)tx];
                if ((double)r.p_hi < u0 + v0 || (double)r.p_lo > u1 + v1 || (double)r.m_hi < u0 - v1 || (double)r.m_lo > u1 - v0) continue;
            }
            const size_t t = (size_t)ty * g.tx_n + tx;
            bits[t >> 5] |= 1u << (t & 31);
        }
    }
}

// One box: grown, its region proposed and proven, rasterised into `bits`.  false: the box is not a box, or its region could not be
// proven or holds a NaN — no bitmap for this stage.  A box proven invisible sets nothing and is true.
inline bool add_box(const rpt_object &ob, int interval, const float o[3], const float box[6], double slope, double L, const Frame &f, const Grid &g, uint32_t *bits) {
    float gb[6];
    if (!grown_box(o, box, slope, L, gb)) return false;
    const Rect r = certified_object_rect(ob, interval, gb);          // proposed, then PROVEN or the full plane
    if (r.u0 <= -3.0e38f && r.v0 <= -3.0e38f && r.u1 >= 3.0e38f && r.v1 >= 3.0e38f && !has_diagonals(r)) return false;
    if (!(r.u0 <= r.u1) || !(r.v0 <= r.v1))
        return !(r.u0 != r.u0 || r.u1 != r.u1 || r.v0 != r.v0 || r.v1 != r.v1);      // (a NaN keeps its object in the kernel: no bitmap); else proven invisible
    rasterise(r, f.diagonals && has_diagonals(r), g, bits);
    return true;
}

inline bool build_arguments_ok(const rpt_object &ob, const float *boxes, int n_boxes, double slope, double L, const Frame &f) {
    if (ob.type != RPT_MESH || n_boxes < 1 || !boxes || f.width < 1 || f.height < 1 || !(slope >= 0.0) || !(slope <= 0.25) || !std::isfinite(L)) return false;
    return f.lens_scale > 0.0f && f.lens_scale <= 1.0f;
}

inline void count_stats(const uint32_t *bits, int n_boxes, const Frame &f, Stats *stats) {
    if (!stats) return;
    int set = 0;
    for (size_t k = 0, words = bitmap_words(f.width, f.height); k < words; k++) set += __builtin_popcount(bits[k]);
    *stats = Stats{n_boxes, n_boxes, set, ((f.width + 7) / 8) * ((f.height + 7) / 8)};
}

// The bitmap of mesh object `ob` (`bits`: bitmap_words() dwords, bit ty * tiles_x + tx of the frame's 8x8 tiles) from ONE stage's
// boxes: `boxes`, n_boxes sub-tree boxes or triangle boxes of its mesh; `slope` = 16.2 K + 3.2u and `L` of that mesh (the caller has
// checked slope <= 0.25).  false: no bitmap — a box that is not a box, or one whose region could not be proven (every bit would be set:
// nothing to gain).
inline bool build(const rpt_object &ob, int interval, const float *boxes, int n_boxes, double slope, double L, const Frame &f,
                  uint32_t *bits, Stats *stats = nullptr) {
    if (stats) *stats = Stats{n_boxes, 0, 0, 0};
    if (!build_arguments_ok(ob, boxes, n_boxes, slope, L, f)) return false;
    const size_t words = bitmap_words(f.width, f.height);
    for (size_t k = 0; k < words; k++) bits[k] = 0u;
    const Grid g(f);
    float o[3];
    cert::kernel_origin(ob, o);
    for (int b = 0; b < n_boxes; b++)
        if (!add_box(ob, interval, o, boxes + 6 * b, slope, L, f, g, bits)) return false;
    count_stats(bits, n_boxes, f, stats);
    return true;
}

// build() with the boxes' proofs shared out to the helper threads (rpt_workers.hpp): the proofs are independent per box, so the boxes
// go out in runs, every run fills a bitmap of its own and the bitmaps are ORed at the end — the same bits whoever proved what, with
// no helpers as with sixteen.  A run that meets a box without a proof stops the others early; the answer is false either way.
inline bool build_pooled(const rpt_object &ob, int interval, const float *boxes, int n_boxes, double slope, double L, const Frame &f,
                         uint32_t *bits, Stats *stats = nullptr) {
    constexpr int RUN_MIN = 64;         // boxes per run at least: below that a run's own bitmap (16 KB at 4K) costs more than its proofs
    rpth::Workers &pool = rpth::Workers::instance();
    const int runs = std::min((n_boxes + RUN_MIN - 1) / RUN_MIN, 4 * (pool.threads() + 1));
    if (runs <= 1 || pool.threads() == 0) return build(ob, interval, boxes, n_boxes, slope, L, f, bits, stats);
    if (stats) *stats = Stats{n_boxes, 0, 0, 0};
    if (!build_arguments_ok(ob, boxes, n_boxes, slope, L, f)) return false;
    const size_t words = bitmap_words(f.width, f.height);
    struct Shared {
        const rpt_object *ob;
        int interval, n_boxes, runs;
        const float *boxes;
        double slope, L;
        const Frame *f;
        const Grid *g;
        float o[3];
        size_t words;
        std::vector<uint32_t> own;          // runs x words, zeroed
        std::atomic<bool> failed{false};
    } sh;
    const Grid g(f);
    sh.ob = &ob; sh.interval = interval; sh.n_boxes = n_boxes; sh.runs = runs; sh.boxes = boxes; sh.slope = slope; sh.L = L; sh.f = &f; sh.g = &g; sh.words = words;
    cert::kernel_origin(ob, sh.o);
    sh.own.assign((size_t)runs * words, 0u);
    pool.parallel_for(runs, [](void *arg, int run) {
        Shared &s = *(Shared *)arg;
        const int b0 = (int)((long long)s.n_boxes * run / s.runs), b1 = (int)((long long)s.n_boxes * (run + 1) / s.runs);
        uint32_t *mine = s.own.data() + (size_t)run * s.words;
        for (int b = b0; b < b1 && !s.failed.load(std::memory_order_relaxed); b++)
            if (!add_box(*s.ob, s.interval, s.o, s.boxes + 6 * b, s.slope, s.L, *s.f, *s.g, mine)) s.failed.store(true);
    }, &sh);
    if (sh.failed.load()) return false;
    for (size_t k = 0; k < words; k++) {
        uint32_t w = 0u;
        for (int run = 0; run < runs; run++) w |= sh.own[(size_t)run * words + k];
        bits[k] = w;
    }
    count_stats(bits, n_boxes, f, stats);
    return true;
}

}  // namespace tiles
}  // namespace rptb
