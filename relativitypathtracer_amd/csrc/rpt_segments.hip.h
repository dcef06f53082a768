// rpt_segments.hip.h — the segment pass (rpt_set_segments / rpt_render_segments; not in the reference): straight rods at
// rest in the rest frame of one object, drawn as a continuum of particles.  A rod is cut into P = pieces equal parts; its P + 1 nodes are
// placed by the particle pass's rules 1-4 (particle_place<false>, as it stands); between two placed nodes the image is the chord, sampled
// about once per pixel, every sample splatted as a particle is (kernel 1140, a scatter into the star pass's accumulator), and kernel
// 1131 resolves.  tests/native/segments_oracle.c restates every rule in C.
#pragma once

#include "rpt_particles.hip.h"

#pragma clang fp contract(off)

namespace rptd {

struct SegmentArgs {
    ParticleArgs p;                     // as the particle pass fills it; p.particles is null, p.count the number of SEGMENTS
    const rpt_segment *segments;        // [p.count] 48 B each
    int pieces;                         // P: 1, 2, 4, ..., 64
    int shift;                          // log2 P
    float period;                       // equirect: Px = (float)W * (two_pi_f / h_fov)
};

// One piece between two placed nodes, as rule S2 leaves it: what rule S3 interpolates.  m == 0: the piece was dropped.
struct SegmentPiece {
    float X0, dX, Y0, dY, dist0, ddist;
    f3 c0, dc;
    float q;                            // len / (float)m
    int m;
};

// Rule S2 from two placed nodes
RPT_DEV void segment_piece(const SegmentArgs &a, float len, float X0, float Y0, float dist0, f3 c0, float X1, float Y1, float dist1, f3 c1, SegmentPiece &o) {
    if (a.p.camera == RPT_STARS_EQUIRECT) {              // the short way round
        if (X1 - X0 > 0.5f * a.period) X1 -= a.period;
        if (X1 - X0 < -0.5f * a.period) X1 += a.period;
    }
    o.X0 = X0;
    o.dX = X1 - X0;
    o.Y0 = Y0;
    o.dY = Y1 - Y0;
    o.dist0 = dist0;
    o.ddist = dist1 - dist0;
    o.c0 = c0;
    o.dc = c1 - c0;
    const float L = fmaxf(fabsf(o.dX), fabsf(o.dY));
    o.m = 0;
    o.q = 0.0f;
    if (!(L <= (float)RPT_SEGMENT_MAX_STEPS)) return;    // (a NaN fails)
    const int m = (int)__builtin_ceilf(L);
    o.m = m < 1 ? 1 : m;
    o.q = len / (float)o.m;
}

// Rules S3 and S4 for sample s of a piece: true = at least one tap is inside the frame and passes the depth test (splat_taps)
RPT_DEV bool segment_sample(const ParticleArgs &a, const SegmentPiece &e, int s) {
    const float u = ((float)s + 0.5f) / (float)e.m;
    const float X = e.X0 + e.dX * u;
    const float Y = e.Y0 + e.dY * u;
    const float dist = e.dist0 + e.ddist * u;
    const f3 c = mk3((e.c0.x + e.dc.x * u) * e.q, (e.c0.y + e.dc.y * u) * e.q, (e.c0.z + e.dc.z * u) * e.q);
    return splat_taps(a, X, Y, dist, c);
}

// Rules S0-S2 for global lane g = segment g / P, piece g % P: the three 16-byte loads of the record, the 80 bytes of InvLorentz and
// stationaryCam as 1130 reads them, the index held against object_count before anything follows it.  NODES ONCE: a lane places node
// j = piece and takes node j + 1 from the lane above it by a cross-lane move (P divides 64, so a segment's pieces lie in one wave);
// the last lane of a segment places b itself.  Every lane of the wave must call this (the moves read every lane).
RPT_DEV void segment_lane_piece(const SegmentArgs &a, int g, SegmentPiece &e) {
    const int P = a.pieces;
    const int segment = g >> a.shift, piece = g & (P - 1);
    e.X0 = e.dX = e.Y0 = e.dY = e.dist0 = e.ddist = e.q = 0.0f;      // a piece that is not placed: all zero, m == 0 (it owns no step)
    e.c0 = e.dc = mk3(0.0f, 0.0f, 0.0f);
    e.m = 0;
    bool live = segment < a.p.count;
    bool placed0 = false, placed1 = false;
    float X0 = 0.0f, Y0 = 0.0f, dist0 = 0.0f, X1 = 0.0f, Y1 = 0.0f, dist1 = 0.0f, len = 0.0f;
    f3 c0 = mk3(0.0f, 0.0f, 0.0f), c1 = c0;
    rpt_float4 inv[4];
    f4 cam = mk4(0.0f, 0.0f, 0.0f, 0.0f);
    f3 end_b = c0, rgb = c0;
    const DObj *window = nullptr;
    if (live) {
        const float4 *record = reinterpret_cast<const float4 *>(a.segments + segment);
        const float4 ra = record[0], rb = record[1], rc = record[2];             // a.xyz, object | b.xyz, padding | rgb.rgb, padding
        const int object = __float_as_int(ra.w);
        live = object >= 0 && object < a.p.object_count;
        if (live) {
            const rpt_object *L = a.p.objects + object;
            for (int k = 0; k < 4; k++) inv[k] = L->InvLorentz[k];
            cam = ld4(L->stationaryCam);
            window = a.p.dobjs ? a.p.dobjs + object : nullptr;
            const f3 end_a = mk3(ra.x, ra.y, ra.z);
            end_b = mk3(rb.x, rb.y, rb.z);
            rgb = mk3(rc.x, rc.y, rc.z);
            const f3 d = end_b - end_a;
            len = __builtin_sqrtf(dot(d, d)) / (float)P;
            live = len > 0.0f && len <= 3.402823466e38f;
            if (live) {
                const f3 pos = end_a + d * ((float)piece / (float)P);
                placed0 = particle_place<false>(a.p, inv, cam, window, pos, rgb, 0.0f, X0, Y0, dist0, c0);
            }
        }
    }
    // node j + 1: the lane above holds it as its node j, unless this lane is its segment's last
    {
        const int up = __shfl_down((int)placed0, 1);
        const float uX = __shfl_down(X0, 1), uY = __shfl_down(Y0, 1), ud = __shfl_down(dist0, 1);
        const float ur = __shfl_down(c0.x, 1), ug = __shfl_down(c0.y, 1), ub = __shfl_down(c0.z, 1);
        if (piece == P - 1) {
            if (live) placed1 = particle_place<false>(a.p, inv, cam, window, end_b, rgb, 0.0f, X1, Y1, dist1, c1);
        } else {
            placed1 = up != 0;
            X1 = uX;
            Y1 = uY;
            dist1 = ud;
            c1 = mk3(ur, ug, ub);
        }
    }
    if (live && placed0 && placed1) segment_piece(a, len, X0, Y0, dist0, c0, X1, Y1, dist1, c1, e);
}

// 1140: one lane per piece for rules S0-S2, then the wave POOLS its steps.  The step counts m of one wave range from 1 to 1024 (a
// lattice in perspective, a rod that passes the camera), so a loop per lane would leave most lanes idle behind the longest piece.
// Instead each lane writes its piece (13 floats and m, a row of 15 words) and the running sum of m to its wave's rows of LDS, the wave forms the inclusive
// prefix sum of m by six cross-lane moves, and lane l takes steps l, l + 64, ... of the pool of T = sum m steps: a binary search of
// the prefix (six LDS reads) finds the step's piece, whose end values are read from LDS.  Consecutive lanes then draw consecutive
// samples — consecutive pixels of one line.  The sums are integers, so the frame is what the lane-per-piece loop gives, bit for bit
// (the diag library's arm, rpt_segments_splat_loop_kernel).  Pieces seen: a flag per piece in LDS (every writer writes 1), then a
// ballot per wave, LDS, one global atomic per workgroup, as 1130.  LDS: 256 pieces x (60 + 4 + 4) B = 17 KiB.
__global__ __launch_bounds__(256) void rpt_segments_splat_kernel(const SegmentArgs a) {
    __shared__ float piece_values[256][15];              // X0 dX Y0 dY dist0 ddist c0 dc q, (int) m; 15 words: odd stride, no bank conflicts
    __shared__ int piece_end[256];                       // inclusive prefix sum of m within the wave
    __shared__ unsigned int piece_seen[256];
    __shared__ unsigned int block_seen;
    const int t = (int)threadIdx.x;
    const int lane = t & 63, base = t & ~63;
    if (t == 0) block_seen = 0u;
    SegmentPiece e;
    segment_lane_piece(a, (int)blockIdx.x * 256 + t, e);
    int end = e.m;
    for (int offset = 1; offset < 64; offset <<= 1) {
        const int below = __shfl_up(end, offset);
        if (lane >= offset) end += below;
    }
    const int total = __shfl(end, 63);
    {
        float *v = piece_values[t];
        v[0] = e.X0; v[1] = e.dX; v[2] = e.Y0; v[3] = e.dY; v[4] = e.dist0; v[5] = e.ddist;
        v[6] = e.c0.x; v[7] = e.c0.y; v[8] = e.c0.z; v[9] = e.dc.x; v[10] = e.dc.y; v[11] = e.dc.z;
        v[12] = e.q; v[13] = __int_as_float(e.m);
        piece_end[t] = end;
        piece_seen[t] = 0u;
    }
    __syncthreads();
    for (int step = lane; step < total; step += 64) {
        int lo = 0;                                      // the first piece of the wave whose inclusive sum exceeds `step`
        for (int half = 32; half > 0; half >>= 1)
            if (piece_end[base + lo + half - 1] <= step) lo += half;
        const int owner = base + lo;                     // lo <= 63: step < total = piece_end[base + 63]
        const float *v = piece_values[owner];
        SegmentPiece o;
        o.X0 = v[0]; o.dX = v[1]; o.Y0 = v[2]; o.dY = v[3]; o.dist0 = v[4]; o.ddist = v[5];
        o.c0 = mk3(v[6], v[7], v[8]);
        o.dc = mk3(v[9], v[10], v[11]);
        o.q = v[12];
        o.m = __float_as_int(v[13]);
        const int s = step - (piece_end[owner] - o.m);
        if (segment_sample(a.p, o, s)) piece_seen[owner] = 1u;
    }
    __syncthreads();
    const unsigned long long set = __ballot(piece_seen[t] != 0u);
    if (lane == 0 && set) atomicAdd(&block_seen, (unsigned int)__popcll(set));
    __syncthreads();
    if (t == 0 && block_seen) atomicAdd(a.p.counts, (unsigned long long)block_seen);
}

#ifdef RPT_DIAGNOSTICS
// The measurement arm of 1140 (librpt_hip_diag.so only; rpt_set_variant 1141): the plain loop, every lane its own piece's m samples.
// Same rules, same integer sums: the same frame and the same counts, bit for bit (tests/test_gpu_segments.py).
__global__ __launch_bounds__(256) void rpt_segments_splat_loop_kernel(const SegmentArgs a) {
    splat_and_count(a.p.counts, [&](int g) {
        SegmentPiece e;
        segment_lane_piece(a, g, e);                     // (every lane: the frame calls the lane function for all of them)
        bool seen = false;
        for (int s = 0; s < e.m; s++) seen |= segment_sample(a.p, e, s);
        return seen;
    });
}
#endif

}  // namespace rptd
