// thermal_host_main.cpp — a stand-alone program over the host side of the thermal point sources that needs no device
// (relativitypathtracer_amd/csrc/rpt_thermal_host.hpp: the temperature array's validation and the conversion T -> x_G), for
// tests/test_thermal_host.py, which builds it plain and with -fsanitize=address,undefined and runs it.  TEST INFRASTRUCTURE ONLY.
// Prints one line "x <T> <x_G>" per converted temperature, both as C99 hexadecimal floats (the test holds them against Python's double
// arithmetic), then "ok <checks>", and returns 0; or the first failed check and 1.
#include <cmath>
#include <cstdio>
#include <limits>
#include <random>
#include <vector>

#include "../../relativitypathtracer_amd/csrc/rpt_thermal_host.hpp"

static int checks = 0;
#define CHECK(cond)                                                     \
    do {                                                                \
        checks++;                                                       \
        if (!(cond)) {                                                  \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond);       \
            return 1;                                                   \
        }                                                               \
    } while (0)

int main() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    // ---- what is accepted: 0, both ends of the range, anything between; a count bounds what is read
    {
        std::vector<float> t = {0.0f, 500.0f, 1e8f, 5772.0f, -0.0f, std::nextafter(500.0f, 1e9f), std::nextafter(1e8f, 0.0f)};
        CHECK(rptt::temperatures_fault(t.data(), (int)t.size()).empty());
        CHECK(rptt::temperatures_fault(t.data(), 0).empty());
        CHECK(rptt::temperatures_fault(nullptr, 0).empty());
        CHECK(rptt::kMaxTemperatures == 1 << 22);
        CHECK(rptt::kMinKelvin == 500.0f && rptt::kMaxKelvin == 1e8f);
    }
    // ---- refusals: the count, a null array, an entry that is not finite, an entry outside the range — each names its entry
    {
        std::vector<float> t = {3000.0f, 6000.0f, 9000.0f};
        CHECK(!rptt::temperatures_fault(t.data(), -1).empty());
        CHECK(!rptt::temperatures_fault(nullptr, rptt::kMaxTemperatures + 1).empty());
        CHECK(rptt::temperatures_fault(nullptr, -1).find("count") == 0);
        CHECK(!rptt::temperatures_fault(nullptr, 1).empty());
        for (float bad : {inf, -inf, nan, std::nextafter(500.0f, 0.0f), std::nextafter(1e8f, 1e9f), 499.0f, 1.0f, 1e-30f, -1.0f, -6000.0f, 3e38f,
                          std::numeric_limits<float>::denorm_min()}) {
            for (int at = 0; at < 3; at++) {
                std::vector<float> d = t;
                d[at] = bad;
                const std::string fault = rptt::temperatures_fault(d.data(), 3);
                CHECK(fault.find("entry " + std::to_string(at) + ":") == 0);
                CHECK(rptt::temperatures_fault(d.data(), at).empty());         // (the count bounds what is read)
            }
        }
        std::vector<float> two = {nan, 10.0f};                                  // the first bad entry is the one named
        CHECK(rptt::temperatures_fault(two.data(), 2).find("entry 0:") == 0);
    }
    // ---- the largest array: validated and converted in place of a device copy
    {
        std::vector<float> big((size_t)rptt::kMaxTemperatures, 5000.0f), out((size_t)rptt::kMaxTemperatures, -1.0f);
        big.back() = 0.0f;
        CHECK(rptt::temperatures_fault(big.data(), rptt::kMaxTemperatures).empty());
        rptt::prepare_temperatures(big.data(), rptt::kMaxTemperatures, out.data());
        CHECK(out.front() == rptt::x_green(5000.0f) && out.back() == 0.0f && out[out.size() - 2] == out.front());
        big[12345] = inf;
        CHECK(rptt::temperatures_fault(big.data(), rptt::kMaxTemperatures).find("entry 12345:") == 0);
    }
    // ---- the conversion: 0 stays 0, x_G falls as T rises, 500 K keeps x_B below 66.1, and the values themselves go to the test
    {
        CHECK(rptt::x_green(0.0f) == 0.0f && rptt::x_green(-0.0f) == 0.0f);
        CHECK(rptt::x_green(500.0f) > rptt::x_green(501.0f) && rptt::x_green(1e8f) > 0.0f);
        CHECK((double)rptt::x_green(500.0f) * (546.1 / 435.8) <= 66.1);
        std::vector<float> t = {500.0f, 1e8f, std::nextafter(500.0f, 1e9f), std::nextafter(1e8f, 0.0f), 3000.0f, 5772.0f, 12000.0f, 1e6f};
        std::mt19937 rng(7);
        std::uniform_real_distribution<double> log_t(std::log(500.0), std::log(1e8));
        for (int i = 0; i < 5000; i++) {
            const float v = (float)std::exp(log_t(rng));
            t.push_back(v < 500.0f ? 500.0f : (v > 1e8f ? 1e8f : v));
        }
        std::vector<float> x(t.size());
        CHECK(rptt::temperatures_fault(t.data(), (int)t.size()).empty());
        rptt::prepare_temperatures(t.data(), (int)t.size(), x.data());
        for (size_t i = 0; i < t.size(); i++) {
            CHECK(x[i] == rptt::x_green(t[i]) && x[i] > 0.0f && std::isfinite(x[i]));
            std::printf("x %a %a\n", (double)t[i], (double)x[i]);
        }
    }
    std::printf("ok %d\n", checks);
    return 0;
}
