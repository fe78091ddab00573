// Host twin of the track descriptor call of local-features_amd/csrc/mkd_track_desc.hip: the kernel's own arithmetic
// (csrc/mkd_track_desc_math.h, compiled here by a plain C++ compiler with -ffp-contract=off) under a serial restatement of the
// walk over a track -- the contributors and the sums of their raw bytes, S and n2, the quantised row, the second walk for the
// spread.  Every sum is an integer sum, so the serial order is the group's and the wave's.  No arithmetic of its own beyond
// the parallax cosine and the scale's default, formed as lf_mkd_track_descriptors_device forms them.
// tests/track_desc_cases.py drives it (built with -fsanitize=address,undefined: a read beyond an array ends the run):
//
//   track_desc_twin IN OUT      IN = calls back to back, OUT = their results back to back
//
//   a call: u64 n_rows, track_capacity, obs_capacity; u32 has_state, min_state, has_points, want_stats; f32 min_parallax_deg,
//       scale; u32 counts[2]; u8 q[n_rows][128]; u64 track_offsets[track_capacity + 1]; i32 obs_row[obs_capacity]; u32
//       obs_state[obs_capacity] if has_state; f32 points[track_capacity][4] if has_points
//   ->  u8 desc[track_capacity][128]; i32 stats[track_capacity][2] if want_stats
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "mkd_track_desc_math.h"

using namespace lfmkd;

namespace {

template <typename T>
void get(FILE *f, T *p, size_t n) {
    if (n && fread(p, sizeof(T), n, f) != n) {
        fprintf(stderr, "track_desc_twin: input ends early\n");
        exit(2);
    }
}
template <typename T>
void put(FILE *f, const T *p, size_t n) {
    if (n && fwrite(p, sizeof(T), n, f) != n) {
        fprintf(stderr, "track_desc_twin: cannot write\n");
        exit(2);
    }
}

uint64_t clamp_to(uint64_t v, uint64_t total) { return v < total ? v : total; }

bool run(FILE *in, FILE *out) {
    uint64_t n_rows;
    if (fread(&n_rows, sizeof n_rows, 1, in) != 1) return false;
    uint64_t tcap, ocap;
    unsigned has_state, min_state, has_points, want_stats, counts[2];
    float deg, scale;
    get(in, &tcap, 1), get(in, &ocap, 1);
    get(in, &has_state, 1), get(in, &min_state, 1), get(in, &has_points, 1), get(in, &want_stats, 1);
    get(in, &deg, 1), get(in, &scale, 1), get(in, counts, 2);
    // exactly as long as the call says, so that the sanitizer sees a read beyond any of them
    std::vector<uint8_t> q(n_rows * kTdRow);
    std::vector<uint64_t> off(tcap + 1);
    std::vector<int32_t> row(ocap);
    std::vector<uint32_t> state(has_state ? ocap : 0);
    std::vector<float> points(has_points ? tcap * 4 : 0);
    get(in, q.data(), q.size()), get(in, off.data(), off.size()), get(in, row.data(), row.size());
    get(in, state.data(), state.size()), get(in, points.data(), points.size());

    if (scale == 0.f) scale = 256.f;
    const double cmin = cos(double(deg) * (3.14159265358979323846 / 180.0));
    const uint64_t T = clamp_to(counts[0], tcap), O = clamp_to(counts[1], ocap);
    std::vector<uint8_t> desc(tcap * kTdRow);
    std::vector<int32_t> stats(want_stats ? tcap * 2 : 0);
    for (uint64_t t = 0; t < tcap; ++t) {
        const bool alive = t < T;
        uint64_t lo = 0, hi = 0;
        if (alive) {
            lo = clamp_to(off[t], O), hi = clamp_to(off[t + 1], O);
            hi = hi > lo ? hi : lo;
        }
        hi = hi - lo > kTdMaxObs ? lo + kTdMaxObs : hi;
        const bool described = alive && td_described(has_points ? points.data() : nullptr, t, cmin);
        const auto contributes = [&](uint64_t k) {
            return td_contributes(has_state != 0, has_state ? state[k] : 0u, min_state, row[k], n_rows);
        };
        uint32_t C = 0, sum[kTdRow] = {};
        for (uint64_t k = lo; k < hi; ++k)
            if (contributes(k)) {
                ++C;
                for (int j = 0; j < kTdRow; ++j) sum[j] += q[uint64_t(row[k]) * kTdRow + j];
            }
        int32_t S[kTdRow], qq[kTdRow];
        int64_t n2 = 0;
        for (int j = 0; j < kTdRow; ++j) S[j] = td_centre(sum[j], C), n2 += td_square(S[j]);
        const bool full = described && C > 0 && n2 > 0;
        const double norm = td_norm(full ? n2 : 1);
        for (int j = 0; j < kTdRow; ++j) {
            qq[j] = full ? td_quantize(S[j], double(scale), norm) : 0;
            desc[t * kTdRow + j] = uint8_t(qq[j] + 128);
        }
        if (want_stats) {
            int32_t spread = kTdNoSpread;
            if (full) {
                spread = INT32_MAX;
                for (uint64_t k = lo; k < hi; ++k)
                    if (contributes(k)) {
                        int32_t d = 0;
                        for (int j = 0; j < kTdRow; ++j) d += td_term(q[uint64_t(row[k]) * kTdRow + j], qq[j]);
                        spread = d < spread ? d : spread;
                    }
            }
            stats[2 * t] = int32_t(C), stats[2 * t + 1] = spread;
        }
    }
    put(out, desc.data(), desc.size()), put(out, stats.data(), stats.size());
    return true;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: track_desc_twin IN OUT\n");
        return 2;
    }
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) {
        fprintf(stderr, "track_desc_twin: cannot open the files\n");
        return 2;
    }
    while (run(in, out)) {}
    fclose(in);
    return fclose(out) == 0 ? 0 : 2;
}
