// rpt_thermal_host.hpp — the part of the thermal point sources (rpt_set_star_temperatures / rpt_set_particle_temperatures)
// that needs no device: the temperature array's validation and the conversion of a temperature to x_G, what the device is given.
// Plain C++17, no HIP: rpt_api.hip includes it, and tests/native/thermal_host_main.cpp compiles it alone (under the address and
// undefined-behaviour sanitizers).
#pragma once

#include <cmath>
#include <string>

namespace rptt {

constexpr int kMaxTemperatures = 1 << 22;       // the catalogue's and the set's own limit
constexpr float kMinKelvin = 500.0f;            // x_B = x_G nu_B <= 66.1: e^x stays a float
constexpr float kMaxKelvin = 1e8f;
constexpr double kHcOverKNm = 1.438776877e7;    // h c / k in nm K, as stars.py carries it
constexpr double kGreenNm = 546.1;

// "" = the array is acceptable; otherwise what the call refuses it for (entry index and value).  An entry is 0 (not thermal: the source
// keeps S_f) or finite with 500 <= T <= 1e8.
inline std::string temperatures_fault(const float *kelvin, int count) {
    if (count < 0 || count > kMaxTemperatures) return "count is 0 .. 2^22 (4194304)";
    if (count > 0 && !kelvin) return "a null array with count > 0";
    for (int i = 0; i < count; i++) {
        const float T = kelvin[i];
        const std::string which = "entry " + std::to_string(i) + ": ";
        if (!std::isfinite(T)) return which + "a temperature must be finite";
        if (T == 0.0f) continue;
        if (!(T >= kMinKelvin) || !(T <= kMaxKelvin)) return which + std::to_string(T) + " K is neither 0 (not thermal) nor within 500 .. 1e8";
    }
    return "";
}

// x_G = (h c / k) / (546.1 nm T), formed in double and rounded to float once; 0 for 0
inline float x_green(float kelvin) {
    if (kelvin == 0.0f) return 0.0f;
    return (float)(kHcOverKNm / (kGreenNm * (double)kelvin));
}

// The array as the device reads it: x_G per source, in the caller's order.  `kelvin` has passed temperatures_fault.
inline void prepare_temperatures(const float *kelvin, int count, float *out) {
    for (int i = 0; i < count; i++) out[i] = x_green(kelvin[i]);
}

}  // namespace rptt
