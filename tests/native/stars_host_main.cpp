// stars_host_main.cpp — a stand-alone program over the host side of the star-field pass that needs no device
// (relativitypathtracer_amd/csrc/rpt_stars_host.hpp: the catalogue's validation and normalisation, and the sky-to-camera
// matrix), for tests/test_stars_host.py, which builds it plain and with -fsanitize=address,undefined and runs it.  TEST INFRASTRUCTURE ONLY.
// Prints "ok <checks>" and returns 0, or the first failed check and 1.
#include <cmath>
#include <cstdio>
#include <limits>
#include <random>
#include <vector>

#include "../../relativitypathtracer_amd/csrc/rpt_stars_host.hpp"

static int checks = 0;
#define CHECK(cond)                                                     \
    do {                                                                \
        checks++;                                                       \
        if (!(cond)) {                                                  \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond);       \
            return 1;                                                   \
        }                                                               \
    } while (0)

static rpt_star star(float x, float y, float z, float r = 1.0f, float g = 1.0f, float b = 1.0f) {
    rpt_star s;
    std::memset(&s, 0, sizeof s);
    s.dir[0] = x; s.dir[1] = y; s.dir[2] = z;
    s.rgb[0] = r; s.rgb[1] = g; s.rgb[2] = b;
    return s;
}

int main() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    // ---- refusals
    {
        std::vector<rpt_star> c = {star(0, 0, 1), star(1, 2, 3)};
        CHECK(rpts::catalogue_fault(c.data(), 2).empty());
        CHECK(rpts::catalogue_fault(c.data(), 0).empty());
        CHECK(!rpts::catalogue_fault(c.data(), -1).empty());
        CHECK(!rpts::catalogue_fault(nullptr, rpts::kMaxStars + 1).empty());
        CHECK(!rpts::catalogue_fault(nullptr, 1).empty());
        for (int k = 0; k < 3; k++)
            for (float bad : {inf, -inf, nan}) {
                std::vector<rpt_star> d = c;
                d[1].dir[k] = bad;
                CHECK(rpts::catalogue_fault(d.data(), 2).find("entry 1") == 0);
                d = c;
                d[0].rgb[k] = bad;
                CHECK(rpts::catalogue_fault(d.data(), 2).find("entry 0") == 0);
            }
        std::vector<rpt_star> d = c;
        d[1] = star(0, 0, 0);
        CHECK(rpts::catalogue_fault(d.data(), 2).find("zero length") != std::string::npos);
        d[1] = star(0, -0.0f, 0);
        CHECK(!rpts::catalogue_fault(d.data(), 2).empty());
        d[1] = star(0, 1, 0, 1.0f, -1e-30f, 1.0f);
        CHECK(rpts::catalogue_fault(d.data(), 2).find("negative") != std::string::npos);
        d[1] = star(0, 1, 0, 0.0f, 0.0f, 0.0f);      // a black star is legal
        CHECK(rpts::catalogue_fault(d.data(), 2).empty());
    }
    // ---- normalisation: the extremes of float do not overflow or vanish
    {
        for (const rpt_star &s : {star(3e38f, 3e38f, 3e38f), star(1e-45f, 0, 0), star(-1e-40f, 1e-40f, 0), star(0.3f, -0.5f, 0.8f)}) {
            float n[3];
            rpts::normalise_direction(s.dir, n);
            const double l = std::sqrt((double)n[0] * n[0] + (double)n[1] * n[1] + (double)n[2] * n[2]);
            CHECK(std::fabs(l - 1.0) < 1e-6);
        }
    }
    // ---- the device's catalogue: the caller's order, unit directions, colours copied, padding zero whatever the caller's held
    {
        std::mt19937 rng(7);
        std::normal_distribution<float> g;
        const int n = 5000;
        std::vector<rpt_star> c;
        for (int i = 0; i < n; i++) {
            c.push_back(star(g(rng) * 1e3f, g(rng) * 1e3f, g(rng) * 1e3f, (float)i, 0.5f, 0.25f));
            c.back()._pad[0] = nan;
            c.back()._pad[1] = 7.0f;
        }
        std::vector<rpt_star> out((size_t)n);
        rpts::prepare_catalogue(c.data(), n, out.data());
        for (int i = 0; i < n; i++) {
            const rpt_star &s = out[(size_t)i];
            CHECK(s.rgb[0] == (float)i && s.rgb[1] == 0.5f && s.rgb[2] == 0.25f && s._pad[0] == 0.0f && s._pad[1] == 0.0f);
            const double l = std::sqrt((double)s.dir[0] * s.dir[0] + (double)s.dir[1] * s.dir[1] + (double)s.dir[2] * s.dir[2]);
            CHECK(std::fabs(l - 1.0) < 1e-6);
            CHECK(s.dir[0] * c[(size_t)i].dir[0] >= 0.0f && s.dir[1] * c[(size_t)i].dir[1] >= 0.0f && s.dir[2] * c[(size_t)i].dir[2] >= 0.0f);
        }
        rpts::prepare_catalogue(c.data(), 0, out.data());      // nothing to do, nothing touched
        rpts::prepare_catalogue(nullptr, 0, nullptr);
    }
    // ---- G: inverse of a boost times a rotation; the spatial block alone with interval 0; singular matrices refused
    {
        const double beta = 0.9, gamma = 1.0 / std::sqrt(1.0 - beta * beta), a = 0.4;
        const double B[16] = {gamma, 0, 0, gamma * beta, 0, 1, 0, 0, 0, 0, 1, 0, gamma * beta, 0, 0, gamma};
        const double R[16] = {1, 0, 0, 0, 0, std::cos(a), 0, std::sin(a), 0, 0, 1, 0, 0, -std::sin(a), 0, std::cos(a)};
        float e[16], g[16];
        for (int r = 0; r < 4; r++)
            for (int c = 0; c < 4; c++) {
                double s = 0;
                for (int k = 0; k < 4; k++) s += B[r * 4 + k] * R[k * 4 + c];
                e[r * 4 + c] = (float)s;
            }
        CHECK(rpts::sky_to_camera(e, -1, g));
        for (int r = 0; r < 4; r++)
            for (int c = 0; c < 4; c++) {
                double s = 0;
                for (int k = 0; k < 4; k++) s += (double)g[r * 4 + k] * e[k * 4 + c];
                CHECK(std::fabs(s - (r == c ? 1.0 : 0.0)) < 1e-5);
            }
        CHECK(rpts::sky_to_camera(e, 0, g));
        CHECK(g[0] == 1.0f && g[1] == 0.0f && g[2] == 0.0f && g[3] == 0.0f && g[4] == 0.0f && g[8] == 0.0f && g[12] == 0.0f);
        for (int r = 1; r < 4; r++)
            for (int c = 1; c < 4; c++) {
                double s = 0;
                for (int k = 1; k < 4; k++) s += (double)g[r * 4 + k] * e[k * 4 + c];
                CHECK(std::fabs(s - (r == c ? 1.0 : 0.0)) < 1e-5);
            }
        float zero[16] = {0};
        CHECK(!rpts::sky_to_camera(zero, -1, g) && !rpts::sky_to_camera(zero, 0, g));
        float twice[16];
        std::memcpy(twice, e, sizeof twice);
        for (int c = 0; c < 4; c++) twice[3 * 4 + c] = twice[1 * 4 + c];      // two equal rows
        CHECK(!rpts::sky_to_camera(twice, -1, g) && !rpts::sky_to_camera(twice, 0, g));
        float time_only[16] = {0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};      // singular as a whole, its spatial block is not
        CHECK(!rpts::sky_to_camera(time_only, -1, g) && rpts::sky_to_camera(time_only, 0, g));
        float huge[16] = {1e-30f, 0, 0, 0, 0, 1e-30f, 0, 0, 0, 0, 1e-30f, 0, 0, 0, 0, 1e-30f};      // invertible in double, G overflows float? no: 1e30 is a float
        CHECK(rpts::sky_to_camera(huge, -1, g) && g[0] == 1e30f);
        float tiny[16] = {1e-44f, 0, 0, 0, 0, 1e-44f, 0, 0, 0, 0, 1e-44f, 0, 0, 0, 0, 1e-44f};      // 1e44 is no finite float
        CHECK(!rpts::sky_to_camera(tiny, -1, g));
    }
    std::printf("ok %d\n", checks);
    return 0;
}
