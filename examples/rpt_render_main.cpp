// rpt_render_main.cpp — a headless C++ host in the shape of the reference's main.cpp:14-74 / render():
// scene DSL on stdin -> upload -> per-frame Lorentz refresh + rpt_set_objects + rpt_render -> PPM.
//
//   g++ -O2 -std=c++17 -Iinclude examples/rpt_render_main.cpp -o rpt_render \
//       -Lrelativitypathtracer_amd -lrpt_hip -lrpt_scene -Wl,-rpath,$PWD/relativitypathtracer_amd
//   ./rpt_render [--yaw D] [--pitch D] [--roll D] [--fov D] [--projection SPEC] [--aa N[:T]] [--events FILE] [--overlay SPEC] [--stars FILE] [--particles SPEC] [--segments SPEC] [--ballistics SPEC] [--rockets SPEC] [--particle-lighting SPEC] [--doppler SPEC] [--star-temperatures FILE] [--particle-temperatures FILE] [--ballistic-temperatures FILE] [--rocket-temperatures FILE] [--glare SPEC] 1920 1080 out.ppm [vx vy vz t [frames in_flight]] < assets/reference/Scenes/shadows.txt
//
// --yaw / --pitch / --roll turn the camera and --fov sets the pinhole's vertical field of view, all in degrees (rpt_set_orientation,
// rpt_set_field_of_view; not in the reference, whose camera looks down +z through a 90-degree lens).  Both are settings of the render
// context, made once, BEFORE the objects are handed over; the per-frame loop stays the reference's.
//
// --projection fisheye[:FOV_DEG[:fit]] | equisolid[:FOV_DEG[:fit]] | stereographic[:FOV_DEG[:fit]] | cube_strip renders through a ray map
// (rpt_raymap_fill, rpt_set_raymap, RPT_PROJECTION_RAYMAP; not in the reference): an equidistant or equisolid fisheye or the stereographic
// view, FOV_DEG degrees across the image circle (default 180), which fit = 0 (the default) inscribes in the frame and fit = 1 stretches to
// its diagonal; or the six faces of a cube side by side (width = 6 height).  Pixels outside the image circle are black.  A setting of
// the render context like the others; it composes with --yaw / --pitch / --roll and excludes --fov and --aa.
//
// --aa N[:T] switches adaptive anti-aliasing on (rpt_set_adaptive_aa; not in the reference): N x N samples in every pixel whose 8-bit
// colour differs from a 4-neighbour's by more than T (default 8; -1 = every pixel) in the one-sample frame.  A setting of the render
// context too; the number of refined pixels goes to stderr.  Without the flag nothing changes.
//
// --events FILE also renders one event pass of the view the PPM shows (rpt_render_events; not in the reference) and writes its raw
// records: width * height * 32 B (rpt_event, rpt_layout.h), row 0 the bottom row as everywhere.  Without the flag nothing changes.
//
// --overlay outlines,clock:STEP,delay:STEP,lattice:SX:SY:SZ,tint[:TMAX] draws lines on the picture before it is written (rpt_set_overlay,
// rpt_render_overlay; not in the reference): any subset of the five layers, in any order — object outlines, contours of the hit object's
// own clock, of the look-back time and of its rest-frame coordinates (a step of 0 skips that axis), and a tint by light delay (TMAX
// omitted: the frame's largest).  The host runs the three passes — the colour frame, an event frame of the same view, the overlay — and
// reports the pixels the overlay changed on stderr.  Without the flag nothing changes.
//
// --stars FILE adds a star field before the picture is written (rpt_set_stars, rpt_render_stars; not in the reference): FILE holds raw
// 32-byte rpt_star records (relativitypathtracer_amd/stars.py `save` writes them) of stars at rest in the scene's frame — the sky's
// frame is set from the scene's camera.  The host runs the colour frame, an event frame of the same view and the star-field pass, under
// the overlay's lines, and reports the stars inside the frame and the pixels changed on stderr.  It excludes --projection (a ray map).
//
// --particles FILE[:inverse_square][:bias=B] adds point sources that ride the scene's objects (rpt_set_particles, rpt_set_particle_options,
// rpt_render_particles; not in the reference): FILE holds raw 32-byte rpt_particle records (relativitypathtracer_amd/particles.py `save`
// writes them), each at rest in the rest frame of the object it names; inverse_square divides a particle's colour by its squared
// rest-frame distance, bias=B (>= 0, in units of distance) lets particles that sit ON a surface show.  The host runs the colour frame, an
// event frame of the same view and the particle pass — behind the stars, under the overlay's lines — and reports the particles seen and
// the pixels changed on stderr.  It excludes --projection (a ray map).
//
// --ballistics FILE[:inverse_square][:bias=B] adds point sources with a velocity of their own (rpt_set_ballistics, rpt_set_ballistic_options,
// rpt_render_ballistics; not in the reference): FILE holds raw 48-byte rpt_ballistic records (relativitypathtracer_amd/ballistics.py `save`
// writes them), each a straight worldline in the rest frame of the object it names; the options as for --particles.  The pass runs behind
// the segments, under the overlay's lines, and the host reports the records seen and the pixels changed.  --ballistic-temperatures FILE:
// raw float32 kelvin, one per record (rpt_set_ballistic_temperatures).
//
// --rockets FILE[:inverse_square][:bias=B] adds point sources under constant proper acceleration (rpt_set_rockets, rpt_set_rocket_options,
// rpt_render_rockets; not in the reference): FILE holds raw 64-byte rpt_rocket records (relativitypathtracer_amd/rockets.py `save` writes
// them), each a hyperbolic worldline in the rest frame of the object it names; the options as for --particles.  The pass runs behind the
// ballistic one, under the overlay's lines, and the host reports the records seen and the pixels changed.  --rocket-temperatures FILE:
// raw float32 kelvin, one per record (rpt_set_rocket_temperatures).
// --particle-lighting lit[,shadows][,ambient] makes the particles of --particles dust (rpt_set_particle_lighting; not in the reference): their
// rgb is an albedo and they show what they scatter from the scene's lights, with light delay on the way from the lamp too; shadows adds
// the renderer's shadow ray per particle and light, ambient the scene's ambient term.  The host reports the pairs lit and shadowed.
//
// --segments FILE[:inverse_square][:bias=B][:pieces=N] adds straight rods that ride the scene's objects (rpt_set_segments,
// rpt_set_segment_options, rpt_render_segments; not in the reference): FILE holds raw 48-byte rpt_segment records
// (relativitypathtracer_amd/segments.py `save` writes them), each rod at rest in the rest frame of the object it names, its colour per unit
// rest-frame length; inverse_square and bias=B as for --particles; pieces=N (1, 2, 4, ..., 64; default 16) is the number of parts a rod is
// cut into — its N + 1 nodes are placed exactly, light delay and all, and joined by chords.  The host runs the colour frame, an event
// frame of the same view and the segment pass — behind the particles, under the overlay's lines — and reports the pieces drawn and the
// pixels changed on stderr.  It excludes --projection (a ray map).
//
// --doppler shift|beaming|both turns the Doppler shift and the searchlight beaming on for every pass (rpt_set_doppler; not in the
// reference).  --star-temperatures FILE and --particle-temperatures FILE make the stars of --stars and the particles of --particles
// thermal sources (rpt_set_star_temperatures, rpt_set_particle_temperatures; not in the reference): FILE holds raw float32 kelvin, one per
// record of the other file in its order, 0 for a source that is none; under --doppler shift or both such a source is shifted as a
// blackbody and is never moved out of the visible band.
//
// --glare W:SIGMA[,W:SIGMA[,W:SIGMA]] gives every point-source pass above a point-spread function (rpt_set_glare; not in the reference):
// up to three Gaussian layers, each carrying the share W (> 0; together at most 1) of a source's flux over SIGMA pixels (0.5 .. 32/3),
// so that a brighter source looks bigger.  Without a pass it spreads it does nothing.
//
// A scene with `dRATE,OFFSET,DIGITS,DECIMALS[,U0,V0,U1,V1]` commands gets its displays drawn too (rpt_set_readouts, rpt_render_readouts;
// not in the reference): seven-segment digits on those objects that show their own time, after the overlay, before the picture is written.
//
// With `frames` > 1 the clock runs (16 ms per frame, as the reference's timer does) and the frames are rendered with
// `in_flight` of them overlapping on the GPU: rpt::FrameRing (include/rpt_frames.hpp) — one context per frame slot
// sharing one resident scene (rpt_share_scene), frame f in slot f mod in_flight.  The PPM is the last frame.
//
// Textures are read with the library's built-in binary PPM reader (convert the JPEGs first, e.g. with
// Pillow) — decoding JPEG is the job of CImg/libjpeg in the reference and is outside the render path.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <iostream>
#include <iterator>
#include <memory>
#include <string>
#include <vector>

#include "rpt.h"
#include "rpt_frames.hpp"
#include "rpt_scene.h"

// --overlay's value into a description with the layers' default colours; false (and a message on stderr) if it cannot be read
static bool parse_overlay(const char *spec, rpt_overlay_desc *d) {
    std::memset(d, 0, sizeof *d);
    const unsigned char white[4] = {255, 255, 255, 255}, yellow[4] = {255, 255, 0, 255}, cyan[4] = {0, 255, 255, 255}, magenta[4] = {255, 0, 255, 255};
    std::memcpy(d->outline_rgba, white, 4);
    std::memcpy(d->delay_rgba, yellow, 4);
    std::memcpy(d->clock_rgba, cyan, 4);
    std::memcpy(d->lattice_rgba, magenta, 4);
    d->tint_alpha = 128;
    const std::string all(spec);
    size_t pos = 0;
    while (pos <= all.size()) {
        const size_t comma = std::min(all.find(',', pos), all.size());
        const std::string item = all.substr(pos, comma - pos);
        pos = comma + 1;
        std::vector<std::string> part;
        for (size_t q = 0; q <= item.size();) {
            const size_t colon = std::min(item.find(':', q), item.size());
            part.push_back(item.substr(q, colon - q));
            q = colon + 1;
        }
        std::vector<float> value;
        for (size_t k = 1; k < part.size(); k++) {
            char *end = nullptr;
            const float v = std::strtof(part[k].c_str(), &end);
            if (part[k].empty() || *end != '\0' || !std::isfinite(v)) {
                std::fprintf(stderr, "--overlay: '%s' in '%s' is not a number\n", part[k].c_str(), item.c_str());
                return false;
            }
            value.push_back(v);
        }
        const std::string &name = part[0];
        const size_t want = name == "outlines" ? 0 : name == "clock" || name == "delay" ? 1 : name == "lattice" ? 3 : name == "tint" ? value.size() <= 1 ? value.size() : 1 : ~(size_t)0;
        if (want == ~(size_t)0) {
            std::fprintf(stderr, "--overlay: unknown layer '%s' (outlines, clock:STEP, delay:STEP, lattice:SX:SY:SZ, tint[:TMAX])\n", name.c_str());
            return false;
        }
        if (value.size() != want) {
            std::fprintf(stderr, "--overlay: '%s' takes %s\n", name.c_str(), name == "outlines" ? "no value" : name == "lattice" ? "three steps, lattice:SX:SY:SZ" : name == "tint" ? "at most one value, tint[:TMAX]" : "one step");
            return false;
        }
        if (name == "outlines") d->layers |= RPT_OVERLAY_OUTLINES;
        else if (name == "clock") { d->layers |= RPT_OVERLAY_ISO_CLOCK; d->clock_step = value[0]; }
        else if (name == "delay") { d->layers |= RPT_OVERLAY_ISO_DELAY; d->delay_step = value[0]; }
        else if (name == "lattice") { d->layers |= RPT_OVERLAY_LATTICE; for (int k = 0; k < 3; k++) d->lattice_step[k] = value[k]; }
        else { d->layers |= RPT_OVERLAY_DELAY_TINT; d->tint_t_max = value.empty() ? 0.0f : value[0]; }
    }
    std::fprintf(stderr, "overlay: layers %u, clock step %g, delay step %g, lattice steps %g %g %g, tint range %g\n", d->layers, d->clock_step, d->delay_step,
                 d->lattice_step[0], d->lattice_step[1], d->lattice_step[2], d->tint_t_max);
    return true;
}

// --projection's value into a filled ray map of width x height; false (and a message on stderr) if it cannot be read or filled
static bool parse_projection(const char *spec, int width, int height, std::vector<float> *dirs) {
    static const char *const usage = "fisheye[:FOV_DEG[:fit]], equisolid[:FOV_DEG[:fit]], stereographic[:FOV_DEG[:fit]] or cube_strip";
    std::vector<std::string> part;
    const std::string all(spec);
    for (size_t q = 0; q <= all.size();) {
        const size_t colon = std::min(all.find(':', q), all.size());
        part.push_back(all.substr(q, colon - q));
        q = colon + 1;
    }
    const std::string &name = part[0];
    const int kind = name == "fisheye" ? RPT_RAYMAP_FISHEYE : name == "equisolid" ? RPT_RAYMAP_FISHEYE_EQUISOLID : name == "stereographic" ? RPT_RAYMAP_STEREOGRAPHIC : name == "cube_strip" ? RPT_RAYMAP_CUBE_STRIP : -1;
    if (kind < 0) {
        std::fprintf(stderr, "--projection: unknown projection '%s' (%s)\n", name.c_str(), usage);
        return false;
    }
    if (part.size() > (kind == RPT_RAYMAP_CUBE_STRIP ? 1u : 3u)) {
        std::fprintf(stderr, "--projection: '%s' has too many values (%s)\n", spec, usage);
        return false;
    }
    float params[2] = {(float)3.14159265358979323846, 0.0f};
    for (size_t k = 1; k < part.size(); k++) {
        char *end = nullptr;
        const double v = std::strtod(part[k].c_str(), &end);
        if (part[k].empty() || *end != '\0' || !std::isfinite(v)) {
            std::fprintf(stderr, "--projection: '%s' in '%s' is not a number\n", part[k].c_str(), spec);
            return false;
        }
        params[k - 1] = k == 1 ? (float)(v * 3.14159265358979323846 / 180.0) : (float)v;
    }
    if (width < 1 || height < 1 || 3ll * width * height >= (1ll << 31)) {
        std::fprintf(stderr, "--projection: no ray map of %d x %d\n", width, height);
        return false;
    }
    dirs->resize((size_t)width * height * 3);
    if (rpt_raymap_fill(kind, kind == RPT_RAYMAP_CUBE_STRIP ? nullptr : params, width, height, dirs->data()) != RPT_OK) {
        if (kind == RPT_RAYMAP_CUBE_STRIP) std::fprintf(stderr, "--projection: cube_strip needs width = 6 height, not %d x %d\n", width, height);
        else std::fprintf(stderr, "--projection: '%s' is out of range (FOV_DEG in (0, 360], below 360 for stereographic; fit 0 or 1)\n", spec);
        return false;
    }
    return true;
}

// --particle-lighting lit[,shadows][,ambient]: the flags of rpt_set_particle_lighting; false (and a message) for what it cannot read.
// (What the library refuses — shadows or ambient without lit — is left to the library, whose message the host prints.)
static bool parse_particle_lighting(const char *spec, int *flags) {
    *flags = 0;
    const std::string s(spec);
    size_t at = 0;
    while (at <= s.size()) {
        const size_t next = s.find(',', at);
        const std::string word = s.substr(at, next == std::string::npos ? std::string::npos : next - at);
        if (word == "lit") *flags |= RPT_PARTICLES_LIT;
        else if (word == "shadows") *flags |= RPT_PARTICLES_SHADOWED;
        else if (word == "ambient") *flags |= RPT_PARTICLES_AMBIENT;
        else {
            std::fprintf(stderr, "--particle-lighting: unknown word '%s' in '%s' (lit, shadows, ambient)\n", word.c_str(), spec);
            return false;
        }
        if (next == std::string::npos) break;
        at = next + 1;
    }
    std::fprintf(stderr, "particle lighting: lit %d, shadows %d, ambient %d\n", !!(*flags & RPT_PARTICLES_LIT), !!(*flags & RPT_PARTICLES_SHADOWED), !!(*flags & RPT_PARTICLES_AMBIENT));
    return true;
}

// --particles / --ballistics / --rockets FILE[:inverse_square][:bias=B] (`noun` = particles / ballistics / rockets): the file name, the flags and the bias;
// false (and a message) for what it cannot read
static bool parse_particles(const char *noun, const char *spec, std::string *path, int *flags, float *bias) {
    const std::string s(spec);
    size_t at = s.find(':');
    *path = s.substr(0, at);
    *flags = 0;
    *bias = 0.0f;
    if (path->empty()) {
        std::fprintf(stderr, "--%s: '%s' names no file\n", noun, spec);
        return false;
    }
    while (at != std::string::npos) {
        const size_t next = s.find(':', at + 1);
        const std::string option = s.substr(at + 1, next == std::string::npos ? std::string::npos : next - at - 1);
        if (option == "inverse_square") *flags |= RPT_PARTICLES_INVERSE_SQUARE;
        else if (option.compare(0, 5, "bias=") == 0) {
            char *end = nullptr;
            const double b = std::strtod(option.c_str() + 5, &end);
            if (end == option.c_str() + 5 || *end != '\0' || !std::isfinite(b) || b < 0.0) {
                std::fprintf(stderr, "--%s: '%s' in '%s' is not a bias (a finite number >= 0)\n", noun, option.c_str() + 5, spec);
                return false;
            }
            *bias = (float)b;
        } else {
            std::fprintf(stderr, "--%s: unknown option '%s' (inverse_square, bias=B)\n", noun, option.c_str());
            return false;
        }
        at = next;
    }
    std::fprintf(stderr, "%s: file %s, inverse square %d, depth bias %g\n", noun, path->c_str(), *flags & RPT_PARTICLES_INVERSE_SQUARE, (double)*bias);
    return true;
}

// --glare W:SIGMA[,W:SIGMA[,W:SIGMA]]: the layers; false (and a message) for what it cannot read or rpt_set_glare would refuse
static bool parse_glare(const char *spec, rpt_glare *glare) {
    std::memset(glare, 0, sizeof *glare);
    const std::string s(spec);
    double total = 0.0;
    size_t at = 0;
    while (true) {
        const size_t next = s.find(',', at);
        const std::string layer = s.substr(at, next == std::string::npos ? std::string::npos : next - at);
        if (glare->layers == RPT_GLARE_LAYERS_MAX) {
            std::fprintf(stderr, "--glare: '%s' has more than %d layers\n", spec, RPT_GLARE_LAYERS_MAX);
            return false;
        }
        char *end = nullptr;
        const double w = std::strtod(layer.c_str(), &end);
        if (end == layer.c_str() || *end != ':' || !(w > 0.0) || !(w <= 1.0)) {
            std::fprintf(stderr, "--glare: '%s' in '%s' is not W:SIGMA with a weight in (0, 1]\n", layer.c_str(), spec);
            return false;
        }
        const char *sigma_text = end + 1;
        const double sigma = std::strtod(sigma_text, &end);
        if (end == sigma_text || *end != '\0' || !(sigma >= 0.5) || !(sigma <= 32.0 / 3.0)) {
            std::fprintf(stderr, "--glare: '%s' in '%s' is not W:SIGMA with a sigma in [0.5, 32/3] pixels\n", layer.c_str(), spec);
            return false;
        }
        glare->weight[glare->layers] = w;
        glare->sigma[glare->layers] = sigma;
        glare->layers++;
        total += std::floor(w * 65536.0 + 0.5);
        if (next == std::string::npos) break;
        at = next + 1;
    }
    if (total > 65536.0) {
        std::fprintf(stderr, "--glare: the weights of '%s' sum to more than 1\n", spec);
        return false;
    }
    std::fprintf(stderr, "glare: %d layers", glare->layers);
    for (int k = 0; k < glare->layers; k++) std::fprintf(stderr, "%s weight %g sigma %g", k ? ";" : ",", glare->weight[k], glare->sigma[k]);
    std::fprintf(stderr, "\n");
    return true;
}

// --segments FILE[:inverse_square][:bias=B][:pieces=N]: the file name, the flags, the bias and the pieces; false (and a message) for
// what it cannot read
static bool parse_segments(const char *spec, std::string *path, int *flags, float *bias, int *pieces) {
    const std::string s(spec);
    size_t at = s.find(':');
    *path = s.substr(0, at);
    *flags = 0;
    *bias = 0.0f;
    *pieces = 16;
    if (path->empty()) {
        std::fprintf(stderr, "--segments: '%s' names no file\n", spec);
        return false;
    }
    while (at != std::string::npos) {
        const size_t next = s.find(':', at + 1);
        const std::string option = s.substr(at + 1, next == std::string::npos ? std::string::npos : next - at - 1);
        if (option == "inverse_square") {
            *flags |= RPT_SEGMENTS_INVERSE_SQUARE;
        } else if (option.compare(0, 5, "bias=") == 0) {
            char *end = nullptr;
            const double b = std::strtod(option.c_str() + 5, &end);
            if (end == option.c_str() + 5 || *end != '\0' || !std::isfinite(b) || b < 0.0) {
                std::fprintf(stderr, "--segments: '%s' in '%s' is not a bias (a finite number >= 0)\n", option.c_str() + 5, spec);
                return false;
            }
            *bias = (float)b;
        } else if (option.compare(0, 7, "pieces=") == 0) {
            char *end = nullptr;
            const long n = std::strtol(option.c_str() + 7, &end, 10);
            if (end == option.c_str() + 7 || *end != '\0' || n < 1 || n > 64 || (n & (n - 1)) != 0) {
                std::fprintf(stderr, "--segments: '%s' in '%s' is not a number of pieces (1, 2, 4, 8, 16, 32 or 64)\n", option.c_str() + 7, spec);
                return false;
            }
            *pieces = (int)n;
        } else {
            std::fprintf(stderr, "--segments: unknown option '%s' (inverse_square, bias=B, pieces=N)\n", option.c_str());
            return false;
        }
        at = next;
    }
    std::fprintf(stderr, "segments: file %s, inverse square %d, depth bias %g, pieces %d\n", path->c_str(), *flags & RPT_SEGMENTS_INVERSE_SQUARE, (double)*bias, *pieces);
    return true;
}

int main(int argc, char **argv) {
    // the free-look options (degrees), taken out of argv; what is left is positional
    float ypr[3] = {0, 0, 0}, v_fov = 0;
    bool turned = false;
    const char *events_path = nullptr, *projection_spec = nullptr, *stars_path = nullptr;
    const char *star_kelvin_path = nullptr, *particle_kelvin_path = nullptr, *ballistic_kelvin_path = nullptr, *rocket_kelvin_path = nullptr;
    int doppler = 0;
    std::string particles_path;
    int particle_flags = 0;
    float particle_bias = 0.0f;
    int particle_lighting = 0;                                   // --particle-lighting
    std::string ballistics_path;                                 // --ballistics
    int ballistic_flags = 0;
    float ballistic_bias = 0.0f;
    std::string rockets_path;                                    // --rockets
    int rocket_flags = 0;
    float rocket_bias = 0.0f;
    std::string segments_path;
    int segment_flags = 0, segment_pieces = 16;
    float segment_bias = 0.0f;
    int aa_n = 1, aa_threshold = 8;
    rpt_glare glare;                                             // --glare
    std::memset(&glare, 0, sizeof glare);
    rpt_overlay_desc overlay;
    std::memset(&overlay, 0, sizeof overlay);
    {
        const double deg = 3.14159265358979323846 / 180.0;
        int kept = 1;
        for (int i = 1; i < argc; i++) {
            const bool has_value = i + 1 < argc;
            if (has_value && !std::strcmp(argv[i], "--yaw")) { ypr[0] = (float)(std::atof(argv[++i]) * deg); turned = true; }
            else if (has_value && !std::strcmp(argv[i], "--pitch")) { ypr[1] = (float)(std::atof(argv[++i]) * deg); turned = true; }
            else if (has_value && !std::strcmp(argv[i], "--roll")) { ypr[2] = (float)(std::atof(argv[++i]) * deg); turned = true; }
            else if (has_value && !std::strcmp(argv[i], "--fov")) v_fov = (float)(std::atof(argv[++i]) * deg);
            else if (has_value && !std::strcmp(argv[i], "--events")) events_path = argv[++i];
            else if (has_value && !std::strcmp(argv[i], "--projection")) projection_spec = argv[++i];
            else if (has_value && !std::strcmp(argv[i], "--stars")) stars_path = argv[++i];
            else if (has_value && !std::strcmp(argv[i], "--star-temperatures")) star_kelvin_path = argv[++i];
            else if (has_value && !std::strcmp(argv[i], "--particle-temperatures")) particle_kelvin_path = argv[++i];
            else if (has_value && !std::strcmp(argv[i], "--ballistic-temperatures")) ballistic_kelvin_path = argv[++i];
            else if (has_value && !std::strcmp(argv[i], "--rocket-temperatures")) rocket_kelvin_path = argv[++i];
            else if (!std::strcmp(argv[i], "--star-temperatures") || !std::strcmp(argv[i], "--particle-temperatures") || !std::strcmp(argv[i], "--ballistic-temperatures") ||
                     !std::strcmp(argv[i], "--rocket-temperatures")) {
                std::fprintf(stderr, "%s needs a file name (raw float32 kelvin, one per record)\n", argv[i]);
                return 2;
            }
            else if (has_value && !std::strcmp(argv[i], "--doppler")) {
                const char *v = argv[++i];
                doppler = !std::strcmp(v, "shift") ? RPT_DOPPLER_SHIFT : !std::strcmp(v, "beaming") ? RPT_DOPPLER_BEAMING
                        : !std::strcmp(v, "both") ? (RPT_DOPPLER_SHIFT | RPT_DOPPLER_BEAMING) : -1;
                if (doppler < 0) {
                    std::fprintf(stderr, "--doppler takes shift, beaming or both\n");
                    return 2;
                }
            } else if (!std::strcmp(argv[i], "--doppler")) {
                std::fprintf(stderr, "--doppler needs a value: shift, beaming or both\n");
                return 2;
            }
            else if (!std::strcmp(argv[i], "--stars")) {
                std::fprintf(stderr, "--stars needs a file name (raw 32-byte rpt_star records)\n");
                return 2;
            }
            else if (has_value && !std::strcmp(argv[i], "--segments")) {
                if (!parse_segments(argv[++i], &segments_path, &segment_flags, &segment_bias, &segment_pieces)) return 2;
            } else if (!std::strcmp(argv[i], "--segments")) {
                std::fprintf(stderr, "--segments needs a value: FILE[:inverse_square][:bias=B][:pieces=N] (raw 48-byte rpt_segment records)\n");
                return 2;
            }
            else if (has_value && !std::strcmp(argv[i], "--particle-lighting")) {
                if (!parse_particle_lighting(argv[++i], &particle_lighting)) return 2;
            } else if (!std::strcmp(argv[i], "--particle-lighting")) {
                std::fprintf(stderr, "--particle-lighting needs a value: lit[,shadows][,ambient]\n");
                return 2;
            }
            else if (has_value && !std::strcmp(argv[i], "--ballistics")) {
                if (!parse_particles("ballistics", argv[++i], &ballistics_path, &ballistic_flags, &ballistic_bias)) return 2;
            } else if (!std::strcmp(argv[i], "--ballistics")) {
                std::fprintf(stderr, "--ballistics needs a value: FILE[:inverse_square][:bias=B] (raw 48-byte rpt_ballistic records)\n");
                return 2;
            }
            else if (has_value && !std::strcmp(argv[i], "--rockets")) {
                if (!parse_particles("rockets", argv[++i], &rockets_path, &rocket_flags, &rocket_bias)) return 2;
            } else if (!std::strcmp(argv[i], "--rockets")) {
                std::fprintf(stderr, "--rockets needs a value: FILE[:inverse_square][:bias=B] (raw 64-byte rpt_rocket records)\n");
                return 2;
            }
            else if (has_value && !std::strcmp(argv[i], "--glare")) {
                if (!parse_glare(argv[++i], &glare)) return 2;
            } else if (!std::strcmp(argv[i], "--glare")) {
                std::fprintf(stderr, "--glare needs a value: W:SIGMA[,W:SIGMA[,W:SIGMA]] (weights > 0 that sum to at most 1, sigmas of 0.5 .. 32/3 pixels)\n");
                return 2;
            }
            else if (has_value && !std::strcmp(argv[i], "--particles")) {
                if (!parse_particles("particles", argv[++i], &particles_path, &particle_flags, &particle_bias)) return 2;
            } else if (!std::strcmp(argv[i], "--particles")) {
                std::fprintf(stderr, "--particles needs a value: FILE[:inverse_square][:bias=B] (raw 32-byte rpt_particle records)\n");
                return 2;
            }
            else if (!std::strcmp(argv[i], "--projection")) {
                std::fprintf(stderr, "--projection needs a value: fisheye[:FOV_DEG[:fit]], equisolid[:FOV_DEG[:fit]], stereographic[:FOV_DEG[:fit]] or cube_strip\n");
                return 2;
            }
            else if (has_value && !std::strcmp(argv[i], "--overlay")) {
                if (!parse_overlay(argv[++i], &overlay)) return 2;
            } else if (!std::strcmp(argv[i], "--overlay")) {
                std::fprintf(stderr, "--overlay needs a value: outlines,clock:STEP,delay:STEP,lattice:SX:SY:SZ,tint[:TMAX]\n");
                return 2;
            }
            else if (has_value && !std::strcmp(argv[i], "--aa")) {
                char *end = nullptr;
                aa_n = (int)std::strtol(argv[++i], &end, 10);
                if (end && *end == ':') aa_threshold = (int)std::strtol(end + 1, &end, 10);
                if (!end || *end != '\0' || end == argv[i]) {
                    std::fprintf(stderr, "--aa takes N or N:T (samples per axis 1..8, threshold -1..255)\n");
                    return 2;
                }
            } else if (!std::strcmp(argv[i], "--aa")) {
                std::fprintf(stderr, "--aa needs a value: N or N:T\n");
                return 2;
            }
            else if (!std::strcmp(argv[i], "--events")) {
                std::fprintf(stderr, "--events needs a file name\n");
                return 2;
            } else if (!std::strcmp(argv[i], "--yaw") || !std::strcmp(argv[i], "--pitch") || !std::strcmp(argv[i], "--roll") || !std::strcmp(argv[i], "--fov")) {
                std::fprintf(stderr, "%s needs a value (degrees)\n", argv[i]);
                return 2;
            } else argv[kept++] = argv[i];
        }
        argc = kept;
    }
    if (argc < 4) {
        std::fprintf(stderr, "usage: %s [--yaw D] [--pitch D] [--roll D] [--fov D] [--projection SPEC] [--aa N[:T]] [--events FILE] [--overlay SPEC] [--stars FILE] [--particles SPEC] [--segments SPEC] [--ballistics SPEC] [--rockets SPEC] [--particle-lighting SPEC] [--doppler SPEC] [--star-temperatures FILE] [--particle-temperatures FILE] [--ballistic-temperatures FILE] [--rocket-temperatures FILE] [--glare SPEC] width height out.ppm [vx vy vz t [frames in_flight]] < scene.txt\n", argv[0]);
        return 2;
    }
    const int width = std::atoi(argv[1]), height = std::atoi(argv[2]);
    std::vector<float> raymap;                                   // --projection: the map, filled on the host (no device needed)
    if (projection_spec && !parse_projection(projection_spec, width, height, &raymap)) return 2;
    std::vector<rpt_star> catalogue;                             // --stars: the raw records
    if (stars_path) {
        std::FILE *f = std::fopen(stars_path, "rb");
        rpt_star s;
        while (f && std::fread(&s, sizeof s, 1, f) == 1) catalogue.push_back(s);
        const bool whole = f && std::feof(f) && std::ftell(f) == (long)(catalogue.size() * sizeof(rpt_star));
        if (f) std::fclose(f);
        if (!whole || catalogue.empty()) {
            std::fprintf(stderr, "--stars: %s does not hold a whole number (> 0) of 32-byte rpt_star records\n", stars_path);
            return 2;
        }
    }
    std::vector<rpt_particle> particle_set;                      // --particles: the raw records
    if (!particles_path.empty()) {
        std::FILE *f = std::fopen(particles_path.c_str(), "rb");
        rpt_particle p;
        while (f && std::fread(&p, sizeof p, 1, f) == 1) particle_set.push_back(p);
        const bool whole = f && std::feof(f) && std::ftell(f) == (long)(particle_set.size() * sizeof(rpt_particle));
        if (f) std::fclose(f);
        if (!whole || particle_set.empty()) {
            std::fprintf(stderr, "--particles: %s does not hold a whole number (> 0) of 32-byte rpt_particle records\n", particles_path.c_str());
            return 2;
        }
    }
    std::vector<rpt_segment> segment_set;                        // --segments: the raw records
    if (!segments_path.empty()) {
        std::FILE *f = std::fopen(segments_path.c_str(), "rb");
        rpt_segment s;
        while (f && std::fread(&s, sizeof s, 1, f) == 1) segment_set.push_back(s);
        const bool whole = f && std::feof(f) && std::ftell(f) == (long)(segment_set.size() * sizeof(rpt_segment));
        if (f) std::fclose(f);
        if (!whole || segment_set.empty()) {
            std::fprintf(stderr, "--segments: %s does not hold a whole number (> 0) of 48-byte rpt_segment records\n", segments_path.c_str());
            return 2;
        }
    }
    std::vector<rpt_ballistic> ballistic_set;                    // --ballistics: the raw records
    if (!ballistics_path.empty()) {
        std::FILE *f = std::fopen(ballistics_path.c_str(), "rb");
        rpt_ballistic b;
        while (f && std::fread(&b, sizeof b, 1, f) == 1) ballistic_set.push_back(b);
        const bool whole = f && std::feof(f) && std::ftell(f) == (long)(ballistic_set.size() * sizeof(rpt_ballistic));
        if (f) std::fclose(f);
        if (!whole || ballistic_set.empty()) {
            std::fprintf(stderr, "--ballistics: %s does not hold a whole number (> 0) of 48-byte rpt_ballistic records\n", ballistics_path.c_str());
            return 2;
        }
    }
    std::vector<rpt_rocket> rocket_set;                          // --rockets: the raw records
    if (!rockets_path.empty()) {
        std::FILE *f = std::fopen(rockets_path.c_str(), "rb");
        rpt_rocket b;
        while (f && std::fread(&b, sizeof b, 1, f) == 1) rocket_set.push_back(b);
        const bool whole = f && std::feof(f) && std::ftell(f) == (long)(rocket_set.size() * sizeof(rpt_rocket));
        if (f) std::fclose(f);
        if (!whole || rocket_set.empty()) {
            std::fprintf(stderr, "--rockets: %s does not hold a whole number (> 0) of 64-byte rpt_rocket records\n", rockets_path.c_str());
            return 2;
        }
    }
    if (particle_lighting && particle_set.empty()) {
        std::fprintf(stderr, "--particle-lighting needs --particles\n");
        return 2;
    }
    std::vector<float> star_kelvin, particle_kelvin, ballistic_kelvin, rocket_kelvin;      // --star-, --particle-, --ballistic-, --rocket-temperatures: raw float32, one per record
    for (int k = 0; k < 4; k++) {
        const char *path = k == 0 ? star_kelvin_path : k == 1 ? particle_kelvin_path : k == 2 ? ballistic_kelvin_path : rocket_kelvin_path;
        const char *flag = k == 0 ? "--star-temperatures" : k == 1 ? "--particle-temperatures" : k == 2 ? "--ballistic-temperatures" : "--rocket-temperatures";
        std::vector<float> &kelvin = k == 0 ? star_kelvin : k == 1 ? particle_kelvin : k == 2 ? ballistic_kelvin : rocket_kelvin;
        const size_t records = k == 0 ? catalogue.size() : k == 1 ? particle_set.size() : k == 2 ? ballistic_set.size() : rocket_set.size();
        if (!path) continue;
        if (records == 0) {
            std::fprintf(stderr, "%s needs %s\n", flag, k == 0 ? "--stars" : k == 1 ? "--particles" : k == 2 ? "--ballistics" : "--rockets");
            return 2;
        }
        std::FILE *f = std::fopen(path, "rb");
        float t;
        while (f && std::fread(&t, sizeof t, 1, f) == 1) kelvin.push_back(t);
        const bool whole = f && std::feof(f) && std::ftell(f) == (long)(kelvin.size() * sizeof(float));
        if (f) std::fclose(f);
        if (!whole || kelvin.size() != records) {
            std::fprintf(stderr, "%s: %s does not hold %zu float32 temperatures, one per record\n", flag, path, records);
            return 2;
        }
    }
    const std::string text((std::istreambuf_iterator<char>(std::cin)), std::istreambuf_iterator<char>());

    rpt_scene *scene = rpt_scene_create();                       // inputScene()            main.cpp:31
    rpt_scene_set_asset_root(scene, std::getenv("RPT_ASSETS") ? std::getenv("RPT_ASSETS") : ".");
    if (rpt_scene_input(scene, text.c_str()) != 0) {
        std::fprintf(stderr, "scene: %s\n", rpt_scene_last_error(scene));
        return 1;
    }
    if (argc >= 8) {
        const float v[3] = {(float)std::atof(argv[4]), (float)std::atof(argv[5]), (float)std::atof(argv[6])};
        const float p[4] = {(float)std::atof(argv[7]), 0, 0, 0};
        rpt_scene_set_camera(scene, v, p);
    }

    rpt_ctx *ctx = nullptr;                                      // initOpenCL()            main.cpp:22
    if (rpt_create(&ctx, 0) != RPT_OK) {
        std::fprintf(stderr, "no usable gfx950 device (the render path has no CPU fallback)\n");
        return 1;
    }
    rpt_scene_desc desc;
    rpt_scene_update_objects(scene);                             // Lorentz block of render() Render.cpp:179-200
    rpt_scene_get_desc(scene, &desc);
    float wp[3], ambient;
    int interval;
    rpt_scene_get_params(scene, wp, &ambient, &interval);
    int rc = RPT_OK;
    if (turned) rc = rpt_set_orientation(ctx, ypr);              // the context's view: before any Object[] is handed over
    if (!rc && v_fov != 0) rc = rpt_set_field_of_view(ctx, v_fov);
    if (!rc && aa_n != 1) rc = rpt_set_adaptive_aa(ctx, aa_n, aa_threshold);
    if (!rc && doppler) rc = rpt_set_doppler(ctx, doppler);
    if (!rc && !raymap.empty()) rc = rpt_set_raymap(ctx, raymap.data(), width, height);
    if (!rc && !raymap.empty()) rc = rpt_set_projection(ctx, RPT_PROJECTION_RAYMAP, nullptr);
    {   // the scene's `wT0,T1` commands (not in the reference): objects and lights that begin and end; a scene without any sets nothing
        size_t n_objects = 0;
        int any_window = 0;
        rpt_scene_get_windows(scene, nullptr, 0, &n_objects, &any_window);
        if (!rc && any_window) {
            std::vector<float> windows(2 * n_objects);
            rpt_scene_get_windows(scene, windows.data(), n_objects, &n_objects, &any_window);
            rc = rpt_set_object_windows(ctx, windows.data(), (int)n_objects);
        }
    }
    if (!rc) rc = rpt_upload_scene(ctx, &desc);                  // 8x cl::Buffer + write    main.cpp:33-55
    if (!rc) rc = rpt_set_params(ctx, wp, ambient, width, height, interval);   // initCLKernel()  main.cpp:62
    if (!rc) rc = rpt_set_output(ctx, nullptr);                  // BufferGL(vbo)           main.cpp:58
    if (!rc) rc = rpt_set_objects(ctx, desc.objects, (int)desc.object_count);   //          Render.cpp:202
    if (!rc) rc = rpt_render(ctx);                               // runKernel()             Render.cpp:205
    if (rc) {
        std::fprintf(stderr, "render: %s\n", rpt_last_error(ctx));
        return 1;
    }
    float ms = 0;
    rpt_last_frame_ms(ctx, &ms);
    rpt_ctx *last = ctx;
    const int frames = argc >= 10 ? std::atoi(argv[8]) : 1, in_flight = argc >= 10 ? std::atoi(argv[9]) : 1;
    std::unique_ptr<rpt::FrameRing> ring_owner;                  // include/rpt_frames.hpp: one context per frame slot, ONE resident scene
    if (frames > 1 && in_flight >= 1) {
        ring_owner.reset(new rpt::FrameRing(0, in_flight));
        rpt::FrameRing &ring = *ring_owner;
        rc = ring.status();
        for (int k = 0; k < ring.frames_in_flight() && !rc; k++) {      // the view is per context: every frame slot gets it
            if (turned) rc = rpt_set_orientation(ring.slot(k), ypr);
            if (!rc && v_fov != 0) rc = rpt_set_field_of_view(ring.slot(k), v_fov);
            if (!rc && aa_n != 1) rc = rpt_set_adaptive_aa(ring.slot(k), aa_n, aa_threshold);
            if (!rc && doppler) rc = rpt_set_doppler(ring.slot(k), doppler);
            if (!rc && !raymap.empty()) rc = rpt_set_raymap(ring.slot(k), raymap.data(), width, height);      // (the map is per context: every slot its copy)
            if (!rc && !raymap.empty()) rc = rpt_set_projection(ring.slot(k), RPT_PROJECTION_RAYMAP, nullptr);
        }
        if (!rc) rc = ring.upload(desc);
        if (!rc) rc = ring.set_params(wp, ambient, width, height, interval);
        rpt_scene_set_paused(scene, 0);
        const auto t0 = std::chrono::steady_clock::now();
        int presented = 0;
        // RPT_DUMP_FRAME=k RPT_DUMP_PATH=file.ppm: also write frame k (0-based) as acquire() handed it out
        const char *dump_path = std::getenv("RPT_DUMP_PATH");
        const int dump_frame = std::getenv("RPT_DUMP_FRAME") ? std::atoi(std::getenv("RPT_DUMP_FRAME")) : -1;
        std::vector<unsigned char> dumped;
        for (int f = 0; f < frames && !rc; f++) {
            rpt_scene_advance_time(scene, 16);                   // render(): cameraPos.x += dt  Render.cpp:177
            rpt_scene_update_objects(scene);
            rpt_scene_get_desc(scene, &desc);
            if (void *finished = ring.acquire()) {               // frame f - in_flight, complete: drawGL() goes here,
                presented++;                                     // BEFORE the slot is resubmitted
                if (dump_path && f - ring.frames_in_flight() == dump_frame) {      // test hook: keep that frame's pixels
                    dumped.resize((size_t)width * height * 16);
                    rc = rpt_read_framebuffer(ring.slot(f % ring.frames_in_flight()), dumped.data(), dumped.size());
                    (void)finished;
                }
            }
            if (!rc) rc = ring.enqueue(desc.objects, (int)desc.object_count);
        }
        if (!rc && ring.drain() == nullptr) rc = ring.status() ? ring.status() : 1;
        if (!rc && dump_path && !dumped.empty()) rc = rpt_write_ppm(dump_path, dumped.data(), width, height);
        const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        if (rc) {
            std::fprintf(stderr, "render: %s\n", ring.last_error());
            return 1;
        }
        last = ring.newest();
        std::fprintf(stderr, "%d frames, %d in flight: %.4f ms/frame, %.0f Mrays/s (%d presented while rendering)\n", frames,
                     ring.frames_in_flight(), sec / frames * 1e3, (double)width * height * frames / sec / 1e6, presented);
    }
    if (glare.layers != 0 && rpt_set_glare(last, &glare) != RPT_OK) {       // every pass below spreads its sources
        std::fprintf(stderr, "glare: %s\n", rpt_last_error(last));
        return 1;
    }
    bool events_rendered = false;
    if (!catalogue.empty()) {                                    // stars on that frame's sky, at rest in the scene's frame
        unsigned long long counts[2] = {0, 0};
        float lorentz[16], inv_lorentz[16];
        rc = rpt_scene_get_camera_lorentz(scene, lorentz, inv_lorentz);
        if (!rc) rc = rpt_set_environment_frame(last, inv_lorentz);
        if (!rc) rc = rpt_render_events(last);
        events_rendered = !rc;
        if (!rc) rc = rpt_set_stars(last, catalogue.data(), (int)catalogue.size());
        if (!rc && !star_kelvin.empty()) rc = rpt_set_star_temperatures(last, star_kelvin.data(), (int)star_kelvin.size());
        if (!rc) rc = rpt_render_stars(last);
        if (!rc) rc = rpt_last_stars(last, counts);
        if (rc) {
            std::fprintf(stderr, "stars: %s\n", rpt_last_error(last));
            return 1;
        }
        std::fprintf(stderr, "stars: %llu of %zu inside the frame, %llu of %lld pixels changed\n", counts[0], catalogue.size(), counts[1], (long long)width * height);
    }
    if (!particle_set.empty()) {                                 // point sources riding the objects, depth-tested against the event frame
        unsigned long long counts[2] = {0, 0};
        rc = events_rendered ? 0 : rpt_render_events(last);
        events_rendered = !rc;
        if (!rc) rc = rpt_set_particles(last, particle_set.data(), (int)particle_set.size());
        if (!rc) rc = rpt_set_particle_options(last, particle_flags, particle_bias);
        if (!rc && !particle_kelvin.empty()) rc = rpt_set_particle_temperatures(last, particle_kelvin.data(), (int)particle_kelvin.size());
        if (!rc) rc = rpt_set_particle_lighting(last, particle_lighting);
        if (!rc) rc = rpt_render_particles(last);
        if (!rc) rc = rpt_last_particles(last, counts);
        unsigned long long pairs[2] = {0, 0};
        if (!rc) rc = rpt_last_particle_lighting(last, pairs);
        if (rc) {
            std::fprintf(stderr, "particles: %s\n", rpt_last_error(last));
            return 1;
        }
        std::fprintf(stderr, "particles: %llu of %zu seen, %llu of %lld pixels changed\n", counts[0], particle_set.size(), counts[1], (long long)width * height);
        if (particle_lighting) std::fprintf(stderr, "particle lighting: %llu (particle, light) pairs lit, %llu shadowed\n", pairs[0], pairs[1]);
    }
    if (!segment_set.empty()) {                                  // rods riding the objects, depth-tested against the event frame
        unsigned long long counts[2] = {0, 0};
        rc = events_rendered ? 0 : rpt_render_events(last);
        events_rendered = !rc;
        if (!rc) rc = rpt_set_segment_options(last, segment_flags, segment_bias, segment_pieces);
        if (!rc) rc = rpt_set_segments(last, segment_set.data(), (int)segment_set.size());
        if (!rc) rc = rpt_render_segments(last);
        if (!rc) rc = rpt_last_segments(last, counts);
        if (rc) {
            std::fprintf(stderr, "segments: %s\n", rpt_last_error(last));
            return 1;
        }
        std::fprintf(stderr, "segments: %llu of %zu pieces drawn, %llu of %lld pixels changed\n", counts[0], segment_set.size() * (size_t)segment_pieces, counts[1], (long long)width * height);
    }
    if (!ballistic_set.empty()) {                                // point sources with their own velocity, depth-tested against the event frame
        unsigned long long counts[2] = {0, 0};
        rc = events_rendered ? 0 : rpt_render_events(last);
        events_rendered = !rc;
        if (!rc) rc = rpt_set_ballistics(last, ballistic_set.data(), (int)ballistic_set.size());
        if (!rc) rc = rpt_set_ballistic_options(last, ballistic_flags, ballistic_bias);
        if (!rc && !ballistic_kelvin.empty()) rc = rpt_set_ballistic_temperatures(last, ballistic_kelvin.data(), (int)ballistic_kelvin.size());
        if (!rc) rc = rpt_render_ballistics(last);
        if (!rc) rc = rpt_last_ballistics(last, counts);
        if (rc) {
            std::fprintf(stderr, "ballistics: %s\n", rpt_last_error(last));
            return 1;
        }
        std::fprintf(stderr, "ballistics: %llu of %zu seen, %llu of %lld pixels changed\n", counts[0], ballistic_set.size(), counts[1], (long long)width * height);
    }
    if (!rocket_set.empty()) {                                   // point sources under constant proper acceleration, depth-tested against the event frame
        unsigned long long counts[2] = {0, 0};
        rc = events_rendered ? 0 : rpt_render_events(last);
        events_rendered = !rc;
        if (!rc) rc = rpt_set_rockets(last, rocket_set.data(), (int)rocket_set.size());
        if (!rc) rc = rpt_set_rocket_options(last, rocket_flags, rocket_bias);
        if (!rc && !rocket_kelvin.empty()) rc = rpt_set_rocket_temperatures(last, rocket_kelvin.data(), (int)rocket_kelvin.size());
        if (!rc) rc = rpt_render_rockets(last);
        if (!rc) rc = rpt_last_rockets(last, counts);
        if (rc) {
            std::fprintf(stderr, "rockets: %s\n", rpt_last_error(last));
            return 1;
        }
        std::fprintf(stderr, "rockets: %llu of %zu seen, %llu of %lld pixels changed\n", counts[0], rocket_set.size(), counts[1], (long long)width * height);
    }
    if (overlay.layers) {                                        // lines on that frame, from an event frame of the same view
        unsigned long long changed = 0;
        rc = events_rendered ? 0 : rpt_render_events(last);
        events_rendered = !rc;
        if (!rc) rc = rpt_set_overlay(last, &overlay);
        if (!rc) rc = rpt_render_overlay(last);
        if (!rc) rc = rpt_last_overlay_pixels(last, &changed);
        if (rc) {
            std::fprintf(stderr, "overlay: %s\n", rpt_last_error(last));
            return 1;
        }
        std::fprintf(stderr, "overlay: %llu of %lld pixels changed\n", changed, (long long)width * height);
    }
    {   // the scene's `dRATE,OFFSET,DIGITS,DECIMALS[,U0,V0,U1,V1]` commands (not in the reference): objects that display their own time,
        // drawn on that frame from an event frame of the same view (rpt_set_readouts, rpt_render_readouts); a scene without any sets nothing
        size_t n_objects = 0;
        int any_readout = 0;
        rpt_scene_get_readouts(scene, nullptr, 0, &n_objects, &any_readout);
        if (any_readout) {
            std::vector<rpt_readout> readouts(n_objects);
            unsigned long long changed = 0;
            rpt_scene_get_readouts(scene, readouts.data(), n_objects, &n_objects, &any_readout);
            rc = events_rendered ? 0 : rpt_render_events(last);
            events_rendered = !rc;
            if (!rc) rc = rpt_set_readouts(last, readouts.data(), (int)n_objects);
            if (!rc) rc = rpt_render_readouts(last);
            if (!rc) rc = rpt_last_readout_pixels(last, &changed);
            if (rc) {
                std::fprintf(stderr, "readouts: %s\n", rpt_last_error(last));
                return 1;
            }
            std::fprintf(stderr, "readouts: %llu of %lld pixels changed\n", changed, (long long)width * height);
        }
    }
    std::vector<unsigned char> fb((size_t)width * height * 16);
    rpt_read_framebuffer(last, fb.data(), fb.size());
    rc = rpt_write_ppm(argv[3], fb.data(), width, height);       // drawGL()                gl_interop.cpp:51
    if (!rc && aa_n != 1) {
        unsigned long long refined = 0;
        rc = rpt_last_aa_refined(last, &refined);
        std::fprintf(stderr, "adaptive anti-aliasing %d x %d, threshold %d: %llu of %lld pixels refined (kernel %d)\n", aa_n, aa_n, aa_threshold, refined,
                     (long long)width * height, rpt_last_aa_variant(last));
    }
    if (!rc && events_path) {                                    // what each pixel of that frame shows, where and when
        std::vector<rpt_event> records((size_t)width * height);
        if (!events_rendered) rc = rpt_render_events(last);      // (--overlay or the scene's readouts have rendered that very frame already)
        if (!rc) rc = rpt_read_events(last, records.data(), records.size() * sizeof(rpt_event));
        if (rc) {
            std::fprintf(stderr, "events: %s\n", rpt_last_error(last));
            return 1;
        }
        std::FILE *f = std::fopen(events_path, "wb");
        if (!f || std::fwrite(records.data(), sizeof(rpt_event), records.size(), f) != records.size() || std::fclose(f) != 0) {
            std::fprintf(stderr, "events: cannot write %s\n", events_path);
            return 1;
        }
    }
    std::fprintf(stderr, "%dx%d frame in %.3f ms -> %s\n", width, height, ms, argv[3]);
    rpt_destroy(ctx);
    rpt_scene_destroy(scene);
    return rc;
}
