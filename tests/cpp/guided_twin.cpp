// Host twin of guided matching's admissibility test: local-features_amd/csrc/mkd_guided_math.h -- the very header the
// kernel match_small_guided_pairs includes -- under a plain C++ compiler (g++ -std=c++17 -O2 -ffp-contract=off -I csrc).
//
//   guided_twin <in> <out>
//
// <in>: problems back to back, each  u32 kind (0 homography, 1 fundamental), u32 na, u32 nb, f32 threshold, f32 model[9],
// f32 a[na][2], f32 b[nb][2].  <out>, per problem, three byte masks:
//   fwd [na][nb]   the a -> b direction as the kernel hoists it: what depends on a_i once per i, then every b_j
//   rev [nb][na]   the b -> a direction: what depends on b_j once per j, then every a_i -- the same relation, (a_i, b_j)
//   ref [na][nb]   the verifier's own test, not hoisted: h_inlier() of mkd_homography_math.h and f_inlier() of
//                  mkd_fundamental_math.h, called directly
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "mkd_fundamental_math.h"
#include "mkd_guided_math.h"
#include "mkd_homography_math.h"

using namespace lfmkd;

int main(int argc, char **argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: guided_twin <in> <out>\n");
        return 2;
    }
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) {
        fprintf(stderr, "guided_twin: cannot open the files\n");
        return 2;
    }
    uint32_t head[3];
    while (fread(head, 4, 3, in) == 3) {
        const uint32_t kind = head[0], na = head[1], nb = head[2];
        float thr, m[9];
        if (kind > 1 || fread(&thr, 4, 1, in) != 1 || fread(m, 4, 9, in) != 9) {
            fprintf(stderr, "guided_twin: bad problem header\n");
            return 1;
        }
        std::vector<float> a(2 * size_t(na)), b(2 * size_t(nb));
        if (fread(a.data(), 4, a.size(), in) != a.size() || fread(b.data(), 4, b.size(), in) != b.size()) {
            fprintf(stderr, "guided_twin: truncated problem\n");
            return 1;
        }
        const float thr2 = thr * thr;   // as launch_ransac (mkd_verify.hip) forms it
        std::vector<uint8_t> fwd(size_t(na) * nb), rev(size_t(na) * nb), ref(size_t(na) * nb);
        for (uint32_t i = 0; i < na; ++i) {
            const float ax = a[2 * i], ay = a[2 * i + 1];
            const GuideHA ha = guide_h_of_a(m, ax, ay, thr2);
            const GuideFA fa = guide_f_of_a(m, ax, ay);
            for (uint32_t j = 0; j < nb; ++j) {
                const float bx = b[2 * j], by = b[2 * j + 1];
                fwd[size_t(i) * nb + j] = kind == 0 ? guide_h_test(ha, bx, by) : guide_f_test(fa, guide_f_of_b(m, bx, by), thr2);
                ref[size_t(i) * nb + j] = kind == 0 ? h_inlier(m, ax, ay, bx, by, thr2) : f_inlier(m, ax, ay, bx, by, thr2);
            }
        }
        for (uint32_t j = 0; j < nb; ++j) {
            const float bx = b[2 * j], by = b[2 * j + 1];
            const GuideFB fb = guide_f_of_b(m, bx, by);
            for (uint32_t i = 0; i < na; ++i) {
                const float ax = a[2 * i], ay = a[2 * i + 1];
                rev[size_t(j) * na + i] = kind == 0 ? guide_h_test(guide_h_of_a(m, ax, ay, thr2), bx, by)
                                                    : guide_f_test(guide_f_of_a(m, ax, ay), fb, thr2);
            }
        }
        if (fwd.empty()) continue;   // an empty side: three empty masks
        fwrite(fwd.data(), 1, fwd.size(), out);
        fwrite(rev.data(), 1, rev.size(), out);
        fwrite(ref.data(), 1, ref.size(), out);
    }
    fclose(in);
    return fclose(out) == 0 ? 0 : 1;
}
