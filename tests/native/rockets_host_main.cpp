// rockets_host_main.cpp — a stand-alone program over the host side of the rocket pass that needs no device
// (relativitypathtracer_amd/csrc/rpt_rockets_host.hpp: the set's validation, its largest object index and the copy the device reads;
// the options are rptp::options_fault of rpt_particles_host.hpp), for tests/test_rockets_host.py, which builds it plain and with
// -fsanitize=address,undefined and runs it.  TEST INFRASTRUCTURE ONLY.  Prints "ok <checks>" and returns 0, or the first failed check and 1.
#include <cmath>
#include <cstdio>
#include <limits>
#include <random>
#include <vector>

#include "../../relativitypathtracer_amd/csrc/rpt_particles_host.hpp"
#include "../../relativitypathtracer_amd/csrc/rpt_rockets_host.hpp"

static int checks = 0;
#define CHECK(cond)                                                     \
    do {                                                                \
        checks++;                                                       \
        if (!(cond)) {                                                  \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond);       \
            return 1;                                                   \
        }                                                               \
    } while (0)

static rpt_rocket record(float x, float y, float z, int object, float ux = 0.0f, float uy = 0.0f, float uz = 0.0f, float ax = 0.0f, float ay = 0.0f, float az = 0.0f) {
    rpt_rocket p;
    std::memset(&p, 0, sizeof p);
    p.pos[0] = x; p.pos[1] = y; p.pos[2] = z;
    p.object = object;
    p.rgb[0] = 1.0f; p.rgb[1] = 0.5f; p.rgb[2] = 0.25f;
    p.u[0] = ux; p.u[1] = uy; p.u[2] = uz;
    p.acc[0] = ax; p.acc[1] = ay; p.acc[2] = az;
    p.t0 = -std::numeric_limits<float>::infinity();
    p.t1 = std::numeric_limits<float>::infinity();
    return p;
}

int main() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    static_assert(sizeof(rpt_rocket) == 64, "rpt_rocket is 64 B");
    // ---- refusals
    {
        std::vector<rpt_rocket> c = {record(0, 0, 1, 0), record(1, 2, 3, 7, 0.5f, -300.0f, 1000.0f, -1000.0f, 0.25f, 1000.0f)};
        CHECK(rptr::set_fault(c.data(), 2).empty());
        CHECK(rptr::set_fault(c.data(), 0).empty());
        CHECK(rptr::set_fault(nullptr, 0).empty());
        CHECK(!rptr::set_fault(c.data(), -1).empty());
        CHECK(!rptr::set_fault(nullptr, rptr::kMaxRockets + 1).empty());
        CHECK(!rptr::set_fault(nullptr, 1).empty());
        CHECK(rptr::kMaxRockets == 1 << 22);
        for (int k = 0; k < 3; k++)
            for (float bad : {inf, -inf, nan}) {
                std::vector<rpt_rocket> d = c;
                d[1].pos[k] = bad;
                CHECK(rptr::set_fault(d.data(), 2).find("entry 1") == 0);
                CHECK(rptr::set_fault(d.data(), 1).empty());      // (the count bounds what is read)
                d = c;
                d[0].rgb[k] = bad;
                CHECK(rptr::set_fault(d.data(), 2).find("entry 0") == 0);
                d = c;
                d[1].u[k] = bad;
                CHECK(rptr::set_fault(d.data(), 2).find("entry 1") == 0);
                d = c;
                d[1].acc[k] = bad;
                CHECK(rptr::set_fault(d.data(), 2).find("entry 1") == 0 && rptr::set_fault(d.data(), 2).find("finite") != std::string::npos);
            }
        for (int k = 0; k < 3; k++)
            for (float big : {1000.0f, -1000.0f}) {
                std::vector<rpt_rocket> d = c;
                d[0].u[k] = big;                                  // 1000 is the last legal component, either way
                CHECK(rptr::set_fault(d.data(), 2).empty());
                d[0].u[k] = std::nextafter(big, big * 2.0f);
                CHECK(rptr::set_fault(d.data(), 2).find("entry 0") == 0 && rptr::set_fault(d.data(), 2).find("u (gamma * beta) is beyond 1000") != std::string::npos);
                d = c;
                d[0].acc[k] = big;
                CHECK(rptr::set_fault(d.data(), 2).empty());
                d[0].acc[k] = std::nextafter(big, big * 2.0f);
                CHECK(rptr::set_fault(d.data(), 2).find("entry 0") == 0 && rptr::set_fault(d.data(), 2).find("acc (the proper acceleration) is beyond 1000") != std::string::npos);
            }
        std::vector<rpt_rocket> d = c;
        d[1].rgb[1] = -1e-30f;
        CHECK(rptr::set_fault(d.data(), 2).find("negative") != std::string::npos);
        d = c;
        d[1].rgb[0] = d[1].rgb[1] = d[1].rgb[2] = 0.0f;           // a black rocket is legal, and so is one at the origin
        d[1].pos[0] = d[1].pos[1] = d[1].pos[2] = 0.0f;
        CHECK(rptr::set_fault(d.data(), 2).empty());
        d = c;
        d[1].object = -1;
        CHECK(rptr::set_fault(d.data(), 2).find("entry 1: object is negative") == 0);
        d[1].object = std::numeric_limits<int32_t>::min();
        CHECK(!rptr::set_fault(d.data(), 2).empty());
        d[1].object = std::numeric_limits<int32_t>::max();        // any index >= 0 is the launch's to hold against Object[]
        CHECK(rptr::set_fault(d.data(), 2).empty());
        // reserved must be 0
        for (float bad : {1.0f, -1e-30f, inf, nan}) {
            d = c;
            d[1].reserved = bad;
            CHECK(rptr::set_fault(d.data(), 2).find("entry 1: reserved must be 0") == 0);
        }
        // the window: no NaN, and t0 < t1; the infinities are "always"
        d = c;
        d[0].t0 = nan;
        CHECK(rptr::set_fault(d.data(), 2).find("entry 0") == 0);
        d = c;
        d[0].t1 = nan;
        CHECK(rptr::set_fault(d.data(), 2).find("entry 0") == 0);
        d = c;
        d[1].t0 = 2.0f; d[1].t1 = 2.0f;
        CHECK(rptr::set_fault(d.data(), 2).find("entry 1") == 0 && rptr::set_fault(d.data(), 2).find("empty") != std::string::npos);
        d[1].t0 = 3.0f; d[1].t1 = 2.0f;
        CHECK(!rptr::set_fault(d.data(), 2).empty());
        d[1].t0 = inf; d[1].t1 = inf;
        CHECK(!rptr::set_fault(d.data(), 2).empty());
        d[1].t0 = -inf; d[1].t1 = -inf;
        CHECK(!rptr::set_fault(d.data(), 2).empty());
        d[1].t0 = 2.0f; d[1].t1 = std::nextafter(2.0f, 3.0f);
        CHECK(rptr::set_fault(d.data(), 2).empty());
        d[1].t0 = -inf; d[1].t1 = 0.0f;
        CHECK(rptr::set_fault(d.data(), 2).empty());
        d[1].t0 = 0.0f; d[1].t1 = inf;
        CHECK(rptr::set_fault(d.data(), 2).empty());
    }
    // ---- the largest object index
    {
        CHECK(rptr::largest_object(nullptr, 0) == -1);
        std::vector<rpt_rocket> c = {record(0, 0, 1, 3), record(0, 0, 1, 0), record(0, 0, 1, 12), record(0, 0, 1, 5)};
        CHECK(rptr::largest_object(c.data(), 4) == 12);
        CHECK(rptr::largest_object(c.data(), 2) == 3);
        CHECK(rptr::largest_object(c.data() + 1, 1) == 0);
        c[1].object = std::numeric_limits<int32_t>::max();
        CHECK(rptr::largest_object(c.data(), 4) == std::numeric_limits<int32_t>::max());
        std::mt19937 rng(3);
        std::vector<rpt_rocket> many;
        int want = -1;
        for (int i = 0; i < 5000; i++) {
            const int o = (int)(rng() % 1000u);
            want = o > want ? o : want;
            many.push_back(record(0, 0, 1, o));
        }
        CHECK(rptr::largest_object(many.data(), 5000) == want);
    }
    // ---- the device's set: the caller's order, every field copied bit for bit
    {
        std::mt19937 rng(7);
        std::normal_distribution<float> g;
        const int n = 5000;
        std::vector<rpt_rocket> c;
        for (int i = 0; i < n; i++) {
            c.push_back(record(g(rng) * 1e3f, g(rng) * 1e3f, g(rng) * 1e3f, i % 17, g(rng), g(rng), g(rng), g(rng), g(rng), g(rng)));
            c.back().rgb[0] = (float)i;
            c.back().t0 = (i & 1) ? -inf : (float)i;
            c.back().t1 = (i & 2) ? inf : (float)i + 0.5f;
        }
        std::vector<rpt_rocket> out((size_t)n);
        rptr::prepare_set(c.data(), n, out.data());
        for (int i = 0; i < n; i++) CHECK(std::memcmp(&out[(size_t)i], &c[(size_t)i], sizeof(rpt_rocket)) == 0);
        rptr::prepare_set(c.data(), 0, out.data());       // nothing to do, nothing touched
        rptr::prepare_set(nullptr, 0, nullptr);
    }
    // ---- the options: the particle pass's
    {
        CHECK(rptp::options_fault(0, 0.0f).empty());
        CHECK(rptp::options_fault(RPT_PARTICLES_INVERSE_SQUARE, 0.25f).empty());
        CHECK(!rptp::options_fault(2, 0.0f).empty());
        CHECK(!rptp::options_fault(-1, 0.0f).empty());
        CHECK(!rptp::options_fault(0, -1e-30f).empty());
        CHECK(!rptp::options_fault(0, inf).empty());
        CHECK(!rptp::options_fault(1, nan).empty());
    }
    std::printf("ok %d\n", checks);
    return 0;
}
