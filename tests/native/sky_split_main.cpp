// rpts::object_box (csrc/rpt_sky_split.hpp) on rectangle sets read from a file, for tests/test_sky_split_host.py.
//   sky_split_main IN OUT
// IN:  per set, int32 {width, height, count}, then count records of 8 floats (rptb::Rect: u0, v0, u1, v1 and the four diagonal bounds).
// OUT: per set, int32 {any, x0, y0, x1, y1}: object_box's answer and its box of 8x8 tiles.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../relativitypathtracer_amd/csrc/rpt_sky_split.hpp"

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *in = std::fopen(argv[1], "rb"), *out = std::fopen(argv[2], "wb");
    if (!in || !out) return 3;
    int32_t head[3];
    std::vector<rptb::Rect> rects;
    long sets = 0;
    while (std::fread(head, sizeof head, 1, in) == 1) {
        if (head[0] < 1 || head[1] < 1 || head[2] < 0 || head[2] > 4096) return 4;
        rects.resize((size_t)head[2]);
        if (head[2] && std::fread(rects.data(), sizeof(rptb::Rect), rects.size(), in) != rects.size()) return 5;
        int box[4];
        const int32_t any = rpts::object_box(rects.data(), head[2], head[0], head[1], box) ? 1 : 0;
        const int32_t row[5] = {any, box[0], box[1], box[2], box[3]};
        if (std::fwrite(row, sizeof row, 1, out) != 1) return 6;
        sets++;
    }
    std::fclose(in);
    if (std::fclose(out) != 0) return 7;
    std::printf("%ld sets\n", sets);
    return 0;
}
