// particles_host_main.cpp — a stand-alone program over the host side of the particle pass that needs no device
// (relativitypathtracer_amd/csrc/rpt_particles_host.hpp: the set's validation, its largest object index, the copy the device reads and
// the options' validation), for tests/test_particles_host.py, which builds it plain and with -fsanitize=address,undefined and runs it.
// TEST INFRASTRUCTURE ONLY.  Prints "ok <checks>" and returns 0, or the first failed check and 1.
#include <cmath>
#include <cstdio>
#include <limits>
#include <random>
#include <vector>

#include "../../relativitypathtracer_amd/csrc/rpt_particles_host.hpp"

static int checks = 0;
#define CHECK(cond)                                                     \
    do {                                                                \
        checks++;                                                       \
        if (!(cond)) {                                                  \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond);       \
            return 1;                                                   \
        }                                                               \
    } while (0)

static rpt_particle particle(float x, float y, float z, int object, float r = 1.0f, float g = 1.0f, float b = 1.0f) {
    rpt_particle p;
    std::memset(&p, 0, sizeof p);
    p.pos[0] = x; p.pos[1] = y; p.pos[2] = z;
    p.object = object;
    p.rgb[0] = r; p.rgb[1] = g; p.rgb[2] = b;
    return p;
}

int main() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    static_assert(sizeof(rpt_particle) == 32, "rpt_particle is 32 B");
    // ---- refusals
    {
        std::vector<rpt_particle> c = {particle(0, 0, 1, 0), particle(1, 2, 3, 7)};
        CHECK(rptp::set_fault(c.data(), 2).empty());
        CHECK(rptp::set_fault(c.data(), 0).empty());
        CHECK(rptp::set_fault(nullptr, 0).empty());
        CHECK(!rptp::set_fault(c.data(), -1).empty());
        CHECK(!rptp::set_fault(nullptr, rptp::kMaxParticles + 1).empty());
        CHECK(!rptp::set_fault(nullptr, 1).empty());
        CHECK(rptp::kMaxParticles == 1 << 22);
        for (int k = 0; k < 3; k++)
            for (float bad : {inf, -inf, nan}) {
                std::vector<rpt_particle> d = c;
                d[1].pos[k] = bad;
                CHECK(rptp::set_fault(d.data(), 2).find("entry 1") == 0);
                CHECK(rptp::set_fault(d.data(), 1).empty());      // (the count bounds what is read)
                d = c;
                d[0].rgb[k] = bad;
                CHECK(rptp::set_fault(d.data(), 2).find("entry 0") == 0);
            }
        std::vector<rpt_particle> d = c;
        d[1] = particle(0, 1, 0, 0, 1.0f, -1e-30f, 1.0f);
        CHECK(rptp::set_fault(d.data(), 2).find("negative") != std::string::npos);
        d[1] = particle(0, 1, 0, 0, 0.0f, 0.0f, 0.0f);        // a black particle is legal, and so is one at the origin
        CHECK(rptp::set_fault(d.data(), 2).empty());
        d[1] = particle(0, 0, 0, 0);
        CHECK(rptp::set_fault(d.data(), 2).empty());
        d[1] = particle(0, 1, 0, -1);
        CHECK(rptp::set_fault(d.data(), 2).find("entry 1: object is negative") == 0);
        d[1] = particle(0, 1, 0, std::numeric_limits<int32_t>::min());
        CHECK(!rptp::set_fault(d.data(), 2).empty());
        d[1] = particle(0, 1, 0, std::numeric_limits<int32_t>::max());      // any index >= 0 is the launch's to hold against Object[]
        CHECK(rptp::set_fault(d.data(), 2).empty());
        d[1]._pad = nan;                                                    // the padding is not looked at
        CHECK(rptp::set_fault(d.data(), 2).empty());
    }
    // ---- the largest object index
    {
        CHECK(rptp::largest_object(nullptr, 0) == -1);
        std::vector<rpt_particle> c = {particle(0, 0, 1, 3), particle(0, 0, 1, 0), particle(0, 0, 1, 12), particle(0, 0, 1, 5)};
        CHECK(rptp::largest_object(c.data(), 4) == 12);
        CHECK(rptp::largest_object(c.data(), 2) == 3);
        CHECK(rptp::largest_object(c.data() + 1, 1) == 0);
        c[1].object = std::numeric_limits<int32_t>::max();
        CHECK(rptp::largest_object(c.data(), 4) == std::numeric_limits<int32_t>::max());
        std::mt19937 rng(3);
        std::vector<rpt_particle> many;
        int want = -1;
        for (int i = 0; i < 5000; i++) {
            const int o = (int)(rng() % 1000u);
            want = o > want ? o : want;
            many.push_back(particle(0, 0, 1, o));
        }
        CHECK(rptp::largest_object(many.data(), 5000) == want);
    }
    // ---- the device's set: the caller's order, every field copied, padding zero whatever the caller's held
    {
        std::mt19937 rng(7);
        std::normal_distribution<float> g;
        const int n = 5000;
        std::vector<rpt_particle> c;
        for (int i = 0; i < n; i++) {
            c.push_back(particle(g(rng) * 1e3f, g(rng) * 1e3f, g(rng) * 1e3f, i % 17, (float)i, 0.5f, 0.25f));
            c.back()._pad = (i & 1) ? nan : 7.0f;
        }
        std::vector<rpt_particle> out((size_t)n);
        rptp::prepare_set(c.data(), n, out.data());
        for (int i = 0; i < n; i++) {
            const rpt_particle &p = out[(size_t)i], &q = c[(size_t)i];
            CHECK(p.rgb[0] == (float)i && p.rgb[1] == 0.5f && p.rgb[2] == 0.25f && p._pad == 0.0f && p.object == i % 17);
            CHECK(p.pos[0] == q.pos[0] && p.pos[1] == q.pos[1] && p.pos[2] == q.pos[2]);
        }
        rptp::prepare_set(c.data(), 0, out.data());       // nothing to do, nothing touched
        rptp::prepare_set(nullptr, 0, nullptr);
    }
    // ---- the options
    {
        CHECK(rptp::options_fault(0, 0.0f).empty());
        CHECK(rptp::options_fault(RPT_PARTICLES_INVERSE_SQUARE, 0.25f).empty());
        CHECK(rptp::options_fault(0, std::numeric_limits<float>::max()).empty());
        CHECK(rptp::options_fault(0, -0.0f).empty());
        CHECK(!rptp::options_fault(2, 0.0f).empty());
        CHECK(!rptp::options_fault(3, 0.0f).empty());
        CHECK(!rptp::options_fault(-1, 0.0f).empty());
        CHECK(!rptp::options_fault(std::numeric_limits<int>::min(), 0.0f).empty());
        CHECK(!rptp::options_fault(0, -1e-30f).empty());
        CHECK(!rptp::options_fault(0, inf).empty());
        CHECK(!rptp::options_fault(0, -inf).empty());
        CHECK(!rptp::options_fault(1, nan).empty());
    }
    std::printf("ok %d\n", checks);
    return 0;
}
