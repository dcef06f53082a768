// segments_host_main.cpp — a stand-alone program over the host side of the segment pass that needs no device
// (relativitypathtracer_amd/csrc/rpt_segments_host.hpp: the set's validation, its largest object index, the copy the device reads, the
// options' validation and the count x pieces limit), for tests/test_segments_host.py, which builds it plain and with
// -fsanitize=address,undefined and runs it.  TEST INFRASTRUCTURE ONLY.  Prints "ok <checks>" and returns 0, or the first failed check and 1.
#include <cmath>
#include <cstdio>
#include <limits>
#include <random>
#include <vector>

#include "../../relativitypathtracer_amd/csrc/rpt_segments_host.hpp"

static int checks = 0;
#define CHECK(cond)                                                     \
    do {                                                                \
        checks++;                                                       \
        if (!(cond)) {                                                  \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond);       \
            return 1;                                                   \
        }                                                               \
    } while (0)

static rpt_segment rod(float ax, float ay, float az, float bx, float by, float bz, int object, float r = 1.0f, float g = 1.0f, float b = 1.0f) {
    rpt_segment s;
    std::memset(&s, 0, sizeof s);
    s.a[0] = ax; s.a[1] = ay; s.a[2] = az;
    s.b[0] = bx; s.b[1] = by; s.b[2] = bz;
    s.object = object;
    s.rgb[0] = r; s.rgb[1] = g; s.rgb[2] = b;
    return s;
}

int main() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    static_assert(sizeof(rpt_segment) == 48, "rpt_segment is 48 B");
    static_assert(RPT_SEGMENT_MAX_STEPS == 1024 && RPT_SEGMENTS_INVERSE_SQUARE == 1, "the two constants");
    // ---- refusals
    {
        std::vector<rpt_segment> c = {rod(0, 0, 1, 0, 1, 1, 0), rod(1, 2, 3, 4, 5, 6, 7)};
        CHECK(rptg::set_fault(c.data(), 2, 16).empty());
        CHECK(rptg::set_fault(c.data(), 0, 16).empty());
        CHECK(rptg::set_fault(nullptr, 0, 64).empty());
        CHECK(!rptg::set_fault(c.data(), -1, 16).empty());
        CHECK(!rptg::set_fault(nullptr, 1, 16).empty());
        CHECK(rptg::kMaxPieces == 1ll << 21 && rptg::kDefaultPieces == 16);
        for (int k = 0; k < 3; k++)
            for (float bad : {inf, -inf, nan}) {
                std::vector<rpt_segment> d = c;
                d[1].a[k] = bad;
                CHECK(rptg::set_fault(d.data(), 2, 16).find("entry 1") == 0);
                CHECK(rptg::set_fault(d.data(), 1, 16).empty());      // (the count bounds what is read)
                d = c;
                d[1].b[k] = bad;
                CHECK(rptg::set_fault(d.data(), 2, 16).find("entry 1") == 0);
                d = c;
                d[0].rgb[k] = bad;
                CHECK(rptg::set_fault(d.data(), 2, 16).find("entry 0") == 0);
            }
        std::vector<rpt_segment> d = c;
        d[1] = rod(0, 1, 0, 0, 2, 0, 0, 1.0f, -1e-30f, 1.0f);
        CHECK(rptg::set_fault(d.data(), 2, 16).find("negative") != std::string::npos);
        d[1] = rod(0, 1, 0, 0, 1, 0, 0, 0.0f, 0.0f, 0.0f);      // a black rod is legal, and so is one of no length (the pass skips it)
        CHECK(rptg::set_fault(d.data(), 2, 16).empty());
        d[1] = rod(0, 1, 0, 1, 1, 0, -1);
        CHECK(rptg::set_fault(d.data(), 2, 16).find("entry 1: object is negative") == 0);
        d[1] = rod(0, 1, 0, 1, 1, 0, std::numeric_limits<int32_t>::min());
        CHECK(!rptg::set_fault(d.data(), 2, 16).empty());
        d[1] = rod(0, 1, 0, 1, 1, 0, std::numeric_limits<int32_t>::max());      // any index >= 0 is the launch's to hold against Object[]
        CHECK(rptg::set_fault(d.data(), 2, 16).empty());
        d[1]._pad0 = nan;                                                       // the padding is not looked at
        d[1]._pad1 = inf;
        CHECK(rptg::set_fault(d.data(), 2, 16).empty());
    }
    // ---- count x pieces <= 2^21, before anything of the set is read
    {
        for (int pieces : {1, 2, 4, 8, 16, 32, 64}) {
            const int most = (int)(rptg::kMaxPieces / pieces);
            CHECK(rptg::load_fault(most, pieces).empty());
            CHECK(!rptg::load_fault(most + 1, pieces).empty());
            CHECK(rptg::set_fault(nullptr, most + 1, pieces).find("count * pieces") == 0);
            CHECK(rptg::options_fault(0, 0.0f, pieces, most).empty());
            CHECK(rptg::options_fault(0, 0.0f, pieces, most + 1).find("count * pieces") == 0);
        }
        CHECK(!rptg::load_fault(std::numeric_limits<int>::max(), 64).empty());     // (the product is formed in 64 bits)
        CHECK(rptg::load_fault(0, 64).empty());
    }
    // ---- the largest object index
    {
        CHECK(rptg::largest_object(nullptr, 0) == -1);
        std::vector<rpt_segment> c = {rod(0, 0, 1, 0, 0, 2, 3), rod(0, 0, 1, 0, 0, 2, 0), rod(0, 0, 1, 0, 0, 2, 12), rod(0, 0, 1, 0, 0, 2, 5)};
        CHECK(rptg::largest_object(c.data(), 4) == 12);
        CHECK(rptg::largest_object(c.data(), 2) == 3);
        CHECK(rptg::largest_object(c.data() + 1, 1) == 0);
        c[1].object = std::numeric_limits<int32_t>::max();
        CHECK(rptg::largest_object(c.data(), 4) == std::numeric_limits<int32_t>::max());
        std::mt19937 rng(3);
        std::vector<rpt_segment> many;
        int want = -1;
        for (int i = 0; i < 5000; i++) {
            const int o = (int)(rng() % 1000u);
            want = o > want ? o : want;
            many.push_back(rod(0, 0, 1, 0, 0, 2, o));
        }
        CHECK(rptg::largest_object(many.data(), 5000) == want);
    }
    // ---- the device's set: the caller's order, every field copied, padding zero whatever the caller's held
    {
        std::mt19937 rng(7);
        std::normal_distribution<float> g;
        const int n = 5000;
        std::vector<rpt_segment> c;
        for (int i = 0; i < n; i++) {
            c.push_back(rod(g(rng) * 1e3f, g(rng) * 1e3f, g(rng) * 1e3f, g(rng), g(rng), g(rng), i % 17, (float)i, 0.5f, 0.25f));
            c.back()._pad0 = (i & 1) ? nan : 7.0f;
            c.back()._pad1 = (i & 2) ? inf : -3.0f;
        }
        std::vector<rpt_segment> out((size_t)n);
        rptg::prepare_set(c.data(), n, out.data());
        for (int i = 0; i < n; i++) {
            const rpt_segment &p = out[(size_t)i], &q = c[(size_t)i];
            CHECK(p.rgb[0] == (float)i && p.rgb[1] == 0.5f && p.rgb[2] == 0.25f && p._pad0 == 0.0f && p._pad1 == 0.0f && p.object == i % 17);
            CHECK(p.a[0] == q.a[0] && p.a[1] == q.a[1] && p.a[2] == q.a[2] && p.b[0] == q.b[0] && p.b[1] == q.b[1] && p.b[2] == q.b[2]);
        }
        rptg::prepare_set(c.data(), 0, out.data());       // nothing to do, nothing touched
        rptg::prepare_set(nullptr, 0, nullptr);
    }
    // ---- the options
    {
        CHECK(rptg::options_fault(0, 0.0f, 16, 0).empty());
        CHECK(rptg::options_fault(RPT_SEGMENTS_INVERSE_SQUARE, 0.25f, 64, 100).empty());
        CHECK(rptg::options_fault(0, std::numeric_limits<float>::max(), 1, 0).empty());
        CHECK(rptg::options_fault(0, -0.0f, 2, 0).empty());
        CHECK(!rptg::options_fault(2, 0.0f, 16, 0).empty());
        CHECK(!rptg::options_fault(3, 0.0f, 16, 0).empty());
        CHECK(!rptg::options_fault(-1, 0.0f, 16, 0).empty());
        CHECK(!rptg::options_fault(std::numeric_limits<int>::min(), 0.0f, 16, 0).empty());
        CHECK(!rptg::options_fault(0, -1e-30f, 16, 0).empty());
        CHECK(!rptg::options_fault(0, inf, 16, 0).empty());
        CHECK(!rptg::options_fault(0, -inf, 16, 0).empty());
        CHECK(!rptg::options_fault(1, nan, 16, 0).empty());
        for (int pieces = -3; pieces <= 130; pieces++) {
            const bool good = pieces == 1 || pieces == 2 || pieces == 4 || pieces == 8 || pieces == 16 || pieces == 32 || pieces == 64;
            CHECK(rptg::options_fault(0, 0.0f, pieces, 0).empty() == good);
        }
        CHECK(!rptg::options_fault(0, 0.0f, std::numeric_limits<int>::min(), 0).empty());
        CHECK(!rptg::options_fault(0, 0.0f, std::numeric_limits<int>::max(), 0).empty());
        CHECK(!rptg::options_fault(0, 0.0f, 1 << 30, 0).empty());
    }
    std::printf("ok %d\n", checks);
    return 0;
}
