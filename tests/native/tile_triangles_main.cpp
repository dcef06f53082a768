// Stand-alone check of the tile bitmap's two stages (relativitypathtracer_amd/csrc/rpt_tile_bitmap.hpp) and of the build through the
// helper pool (rpt_workers.hpp): a synthetic two-level octree with a dozen triangles, the sub-tree stage and the triangle stage built
// serially and through the pool, compared bit for bit; the triangle stage refines the sub-tree stage; the cap, a NaN vertex and a
// broken index are refused.  Built by tests/test_tile_triangles_native.py, plain and under the address and undefined-behaviour
// sanitizers.  RPT_HOST_THREADS is set by main() itself so that the pool has helpers on any machine.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../relativitypathtracer_amd/csrc/rpt_tile_bitmap.hpp"
#include "../../relativitypathtracer_amd/csrc/rpt_workers.hpp"

namespace {

int failures = 0;
#define CHECK(cond)                                                           \
    do {                                                                      \
        if (!(cond)) {                                                        \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond);             \
            failures++;                                                       \
        }                                                                     \
    } while (0)

struct Mesh {
    std::vector<rpt_float3> vertices;
    std::vector<uint32_t> triangles;
    std::vector<rpt_octree> octrees;
    std::vector<int32_t> octreeTris;
    rpt_object object;
    rpt_scene_desc desc;
};

rpt_float3 f3(float x, float y, float z) { return rpt_float3{x, y, z, 0.0f}; }

// a root with eight leaves over [-0.5, 0.5]^3; twelve small triangles, one or two per octant, two of them listed by two leaves each
void make(Mesh &m) {
    m.octrees.assign(9, rpt_octree{});
    rpt_octree &root = m.octrees[0];
    root.min = f3(-0.5f, -0.5f, -0.5f);
    root.max = f3(0.5f, 0.5f, 0.5f);
    root.trisIndex = 0;
    root.trisCount = 0;
    for (int k = 0; k < 6; k++) root.neighbors[k] = -1;
    for (int c = 0; c < 8; c++) {
        root.children[c] = 1 + c;
        rpt_octree &leaf = m.octrees[(size_t)1 + c];
        const float x0 = (c & 4) ? 0.0f : -0.5f, y0 = (c & 2) ? 0.0f : -0.5f, z0 = (c & 1) ? 0.0f : -0.5f;
        leaf.min = f3(x0, y0, z0);
        leaf.max = f3(x0 + 0.5f, y0 + 0.5f, z0 + 0.5f);
        for (int k = 0; k < 8; k++) leaf.children[k] = -1;
        for (int k = 0; k < 6; k++) leaf.neighbors[k] = -1;
    }
    unsigned seed = 12345u;
    auto rnd = [&seed]() { seed = seed * 1664525u + 1013904223u; return (float)(seed >> 8) / 16777216.0f; };
    std::vector<std::vector<int>> lists(8);
    for (int t = 0; t < 12; t++) {
        const int c = t % 8;
        const rpt_octree &leaf = m.octrees[(size_t)1 + c];
        const float ax = leaf.min.x + 0.1f + 0.25f * rnd(), ay = leaf.min.y + 0.1f + 0.25f * rnd(), az = leaf.min.z + 0.1f + 0.25f * rnd();
        const uint32_t v0 = (uint32_t)m.vertices.size();
        m.vertices.push_back(f3(ax, ay, az));
        m.vertices.push_back(f3(ax + 0.01f * rnd(), ay + 0.01f * rnd(), az));
        m.vertices.push_back(f3(ax, ay + 0.01f * rnd(), az + 0.01f * rnd()));
        for (uint32_t k = 0; k < 3; k++) { m.triangles.push_back(v0 + k); m.triangles.push_back(0u); m.triangles.push_back(0u); }
        lists[(size_t)c].push_back(t);
    }
    lists[1].push_back(0);          // two triangles named twice: the stage counts DISTINCT triangles
    lists[6].push_back(3);
    for (int c = 0; c < 8; c++) {
        m.octrees[(size_t)1 + c].trisIndex = (int32_t)m.octreeTris.size();
        m.octrees[(size_t)1 + c].trisCount = (int32_t)lists[(size_t)c].size();
        for (int t : lists[(size_t)c]) m.octreeTris.push_back(t);
    }
    // the mesh at rest, two units in front of a camera at rest: M = translation, Lorentz = identity
    std::memset(&m.object, 0, sizeof m.object);
    rpt_float4 *mats[4] = {m.object.M, m.object.InvM, m.object.Lorentz, m.object.InvLorentz};
    for (rpt_float4 *mat : mats) {
        mat[0].x = 1.0f; mat[1].y = 1.0f; mat[2].z = 1.0f; mat[3].w = 1.0f;
    }
    m.object.M[2].w = 2.0f;
    m.object.InvM[2].w = -2.0f;
    m.object.type = RPT_MESH;
    m.object.meshIndex = 0;
    m.object.textureIndex = -1;
    std::memset(&m.desc, 0, sizeof m.desc);
    m.desc.objects = &m.object; m.desc.object_count = 1;
    m.desc.vertices = m.vertices.data(); m.desc.vertex_count = m.vertices.size();
    m.desc.triangles = m.triangles.data(); m.desc.triangle_words = m.triangles.size();
    m.desc.octrees = m.octrees.data(); m.desc.octree_count = m.octrees.size();
    m.desc.octreeTris = m.octreeTris.data(); m.desc.octree_tri_count = m.octreeTris.size();
}

int popcount(const std::vector<uint32_t> &bits) {
    int n = 0;
    for (uint32_t w : bits) n += __builtin_popcount(w);
    return n;
}

}  // namespace

int main() {
    setenv("RPT_HOST_THREADS", "4", 1);         // before the pool's first use
    using namespace rptb::tiles;
    Mesh m;
    make(m);
    std::vector<float> cut, tris;
    int depth = -1;
    CHECK(subtree_boxes(m.desc, 0, MAX_BOXES, cut, &depth) && cut.size() == 8 * 6 && depth == 1);
    CHECK(triangle_boxes(m.desc, 0, MAX_TRIANGLES, tris) && tris.size() == 12 * 6);
    // every triangle's box lies in the box of the sub-tree that lists it (triangle t is listed by leaf t % 8; the cut's boxes come in child order)
    for (size_t t = 0; t < tris.size() / 6; t++)
        for (int k = 0; k < 3; k++) CHECK(tris[6 * t + k] >= cut[6 * (t % 8) + k] && tris[6 * t + 3 + k] <= cut[6 * (t % 8) + 3 + k]);
    // refusals
    std::vector<float> none;
    CHECK(!triangle_boxes(m.desc, 0, 11, none) && none.empty());                  // over the cap
    CHECK(triangle_boxes(m.desc, 0, 12, none) && none.size() == 12 * 6);
    CHECK(!triangle_boxes(m.desc, 9, MAX_TRIANGLES, none));                       // no such root
    {
        Mesh bad;
        make(bad);
        bad.vertices[7].y = NAN;
        CHECK(!triangle_boxes(bad.desc, 0, MAX_TRIANGLES, none) && none.empty());
        make(bad = Mesh());
        bad.octreeTris[3] = 12;                                                   // a triangle that does not exist
        CHECK(!triangle_boxes(bad.desc, 0, MAX_TRIANGLES, none));
        make(bad = Mesh());
        bad.octrees[4].children[0] = 0;                                           // a child loop
        for (int k = 1; k < 8; k++) bad.octrees[4].children[k] = 1 + k;
        CHECK(!triangle_boxes(bad.desc, 0, MAX_TRIANGLES, none));
    }

    const double slope = 16.2 * 2.0e-4 + 3.2 * rptb::cert::U24, L = 0.015;        // edges below 0.01 sqrt 2: |e1| |e2| <= 2e-4, well inside the rule
    const Frame frames[3] = {{253, 141, 1.0f, true}, {640, 360, 1.0f, true}, {128, 72, 0.5f, false}};
    for (const Frame &f : frames) {
        const size_t words = bitmap_words(f.width, f.height);
        std::vector<uint32_t> s0(words), s1(words), p0(words), p1(words);
        Stats a{}, b{}, c{}, d{};
        CHECK(build(m.object, -1, cut.data(), (int)(cut.size() / 6), slope, L, f, s0.data(), &a));
        CHECK(build(m.object, -1, tris.data(), (int)(tris.size() / 6), slope, L, f, s1.data(), &b));
        CHECK(build_pooled(m.object, -1, cut.data(), (int)(cut.size() / 6), slope, L, f, p0.data(), &c));
        CHECK(build_pooled(m.object, -1, tris.data(), (int)(tris.size() / 6), slope, L, f, p1.data(), &d));
        CHECK(s0 == p0 && s1 == p1);
        CHECK(a.proven == 8 && b.proven == 12 && c.tiles_set == a.tiles_set && d.tiles_set == b.tiles_set);
        for (size_t k = 0; k < words; k++) CHECK((s1[k] & ~s0[k]) == 0u);       // a triangle's region lies in its sub-tree's
        CHECK(popcount(s1) > 0 && popcount(s1) < popcount(s0));
        std::printf("%dx%d lens %.1f: sub-tree stage %d tiles, triangle stage %d tiles of %d\n", f.width, f.height, (double)f.lens_scale, a.tiles_set, b.tiles_set, a.tiles);
    }

    // many boxes: enough runs for every helper (the dozen above is one run); copies of the triangles' boxes, shifted a little
    {
        std::vector<float> many;
        for (int k = 0; k < 700; k++)
            for (size_t t = 0; t < tris.size() / 6; t++)
                for (int c = 0; c < 6; c++) many.push_back(tris[6 * t + c] + 0.0004f * (float)k * (c % 3 == 0 ? 1.0f : -0.5f));
        const Frame f{640, 360, 1.0f, true};
        const size_t words = bitmap_words(f.width, f.height);
        std::vector<uint32_t> serial(words), pooled(words);
        Stats a{}, b{};
        CHECK(build(m.object, -1, many.data(), (int)(many.size() / 6), slope, L, f, serial.data(), &a));
        for (int round = 0; round < 3; round++) {
            std::fill(pooled.begin(), pooled.end(), 0xffffffffu);
            CHECK(build_pooled(m.object, -1, many.data(), (int)(many.size() / 6), slope, L, f, pooled.data(), &b));
            CHECK(serial == pooled && a.tiles_set == b.tiles_set && b.proven == (int)(many.size() / 6));
        }
        // one box among them that is not a box: no bitmap, serially and through the pool
        many[6 * 5000 + 3] = many[6 * 5000] - 1.0f;
        CHECK(!build(m.object, -1, many.data(), (int)(many.size() / 6), slope, L, f, serial.data()));
        CHECK(!build_pooled(m.object, -1, many.data(), (int)(many.size() / 6), slope, L, f, pooled.data()));
        std::printf("%d boxes: %d tiles set, %d helpers\n", (int)(many.size() / 6), a.tiles_set, rpth::Workers::instance().threads());
    }
    if (failures) return 1;
    std::printf("ok\n");
    return 0;
}
