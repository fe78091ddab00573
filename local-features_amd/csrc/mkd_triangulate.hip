// gfx950 track triangulation (include/lf_mkd.h, lf_mkd_triangulate_tracks_device): per track of a track table
// the 3-D point its observations give under known camera poses -- pair hypotheses among the first usable observations, a
// midpoint least squares over the winner's inliers, trimming rounds, the parallax of the inliers.  The arithmetic is
// csrc/mkd_triangulate_math.h, which the host twin compiles too.
//
//   triangulate_tracks   ONE launch.  A GROUP of kTriSlots = 4 lanes owns a track: 16 tracks a wave, 64 a workgroup.  Lane l
//                        of the group reads the positions lo + l, lo + 4 + l, ... of the track, so the lane IS the slot of
//                        the canonical sum: it adds its positions' contributions in ascending order, and the group combines
//                        the four sums by a butterfly over lane xor 2, 1 (ds_bpermute), which leaves (s0 + s2) + (s1 + s3)
//                        in every lane.  Counts are popcounts of the group's bits of a ballot.  The first 4 positions stay
//                        in registers (observation and ray); a longer track is walked 4 positions at a time and reads the
//                        later ones again on every walk.  Lane l of the group also keeps the contributions of candidates l
//                        and l + 4; a pair hypothesis broadcasts two of them, places them in their slots, combines, solves,
//                        and scores with one walk.  (The mean track of a collection is 3 to 4 long: at 8 lanes per track
//                        half the lanes idle, and the table of 1.3 M pairs takes 1.9 x as long -- profiles/triangulate.md.)
//
// No scratch memory, no LDS, no allocation, no atomic, and no workgroup waits for another.  Every loop that holds a ballot or
// a lane permute runs in wave-uniform control flow: its condition is an __any, and a group that is done goes through the
// steps with its predicate off.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mkd_device.h"
#include "mkd_triangulate_math.h"
#include "mkd_scene.h"   // behind the arithmetic: its walk is kTriSlots lanes wide

namespace lfmkd {
namespace {

constexpr int kThreads = kSumThreads;
constexpr int G = kTriSlots;
constexpr unsigned kMaxBlocks = 16384;                  // grid-stride beyond
constexpr int kSets = kTriCandidates / G;              // candidates a lane keeps: lane l has l and l + 4 (one, at 8 lanes)
static_assert(kSets * G == kTriCandidates, "the candidates fill the group's lanes a whole number of times");

// position k of the observation arrays (k < O): false if it is not usable; else what it reads
__device__ __forceinline__ bool load_obs(const SceneTables &tb, const float *poses, uint64_t k, TriObs &o) {
    const int row = tb.obs_row[k];
    const unsigned img = tb.obs_image[k];
    if (row < 0 || (uint64_t)row >= tb.n_rows || img >= tb.n_images) return false;
#pragma unroll
    for (int i = 0; i < 4; ++i) o.K[i] = tb.intrinsics[4 * (uint64_t)img + i];
#pragma unroll
    for (int i = 0; i < 12; ++i) o.P[i] = poses[12 * (uint64_t)img + i];
    o.x = tb.kps[5 * (uint64_t)row];
    o.y = tb.kps[5 * (uint64_t)row + 1];
    return tri_camera_usable(o.K, o.P) && tri_keypoint_usable(o.x, o.y);
}

}  // namespace

__global__ __launch_bounds__(kThreads) void triangulate_tracks(SceneTables tb, const float *poses, double thr2, unsigned rounds,
                                                               float *__restrict__ points, unsigned *__restrict__ stats,
                                                               float *__restrict__ err, unsigned *__restrict__ obs_state) {
    const TrackWalk walk = track_walk(tb);
    for (uint64_t t0 = walk.first; t0 < walk.T; t0 += walk.stride) {            // wave-uniform
        const uint64_t t = t0 + (threadIdx.x & 63) / G;
        const bool alive = t < walk.T;
        uint64_t lo = 0, hi = 0;
        if (alive) track_range(tb, t, walk.O, lo, hi);
        const unsigned nch = (unsigned)((hi - lo + G - 1) / G);

        // the first chunk stays in registers
        TriObs o0 = {};
        TriRay r0 = {};
        const bool u0 = lo + walk.l < hi && load_obs(tb, poses, lo + walk.l, o0);
        if (u0) tri_ray(o0, r0);
        // position lo + G ch + l under predicate `on`: is it in the track (`in`), usable, and then its observation and ray
        const auto fetch = [&](unsigned ch, bool on, uint64_t &pos, bool &in, TriObs &o, TriRay &r) {
            pos = lo + (uint64_t)ch * G + walk.l;
            in = on && pos < hi;
            if (ch == 0) {
                o = o0;
                r = r0;
                return in && u0;
            }
            const bool usable = in && load_obs(tb, poses, pos, o);
            if (usable) tri_ray(o, r);
            return usable;
        };

        // the usable positions: their number, and candidate l's position in lane l
        unsigned U = 0;
        uint64_t cand[kSets];
#pragma unroll
        for (int q = 0; q < kSets; ++q) cand[q] = 0;
        for (unsigned ch = 0; __any(ch < nch); ++ch) {
            uint64_t pos;
            bool in;
            TriObs o = {};
            TriRay r = {};
            const bool usable = fetch(ch, ch < nch, pos, in, o, r);
            const unsigned m = group_bits(usable, walk.base), before = U;
            U += (unsigned)__popc(m);
#pragma unroll
            for (int set = 0; set < kSets; ++set) {
                const unsigned c = walk.l + set * G;                               // candidate c is this chunk's (c - before)-th usable
                if (c >= before && c < U) {
                    unsigned mm = m;
#pragma unroll
                    for (unsigned q = 0; q < G - 1; ++q) mm = q < c - before ? mm & (mm - 1) : mm;
                    cand[set] = lo + (uint64_t)ch * G + ((unsigned)__ffs((int)mm) - 1u);
                }
            }
        }
        const unsigned ncand = U < kTriCandidates ? U : kTriCandidates;
        unsigned reason = U < 2 ? kTriFewUsable : kTriPoint;
        double cw[kSets][kTriTerms];
        unsigned cslot[kSets];
#pragma unroll
        for (int set = 0; set < kSets; ++set) {
#pragma unroll
            for (int i = 0; i < kTriTerms; ++i) cw[set][i] = 0.0;
            TriObs o = {};
            TriRay r = {};
            if (walk.l + set * G < ncand && load_obs(tb, poses, cand[set], o)) {
                tri_ray(o, r);
                tri_contribution(r, cw[set]);
            }
            cslot[set] = (unsigned)(cand[set] - lo) & (G - 1);
        }
        // candidate c's value: lane c mod G of the group, set c / G (c is wave-uniform, so the set is a uniform select)
        const auto cand_u = [&](const unsigned (&v)[kSets], unsigned c) {
            unsigned x = v[0];
#pragma unroll
            for (int set = 1; set < kSets; ++set) x = c / G == (unsigned)set ? v[set] : x;
            return (unsigned)__shfl((int)x, (int)(walk.base + c % G), 64);
        };
        const auto cand_d = [&](int k, unsigned c) {
            double x = cw[0][k];
#pragma unroll
            for (int set = 1; set < kSets; ++set) x = c / G == (unsigned)set ? cw[set][k] : x;
            return __shfl(x, (int)(walk.base + c % G), 64);
        };

        // step 5: the pair hypotheses
        bool have = false;
        unsigned best = 0, pair = kTriNoPair;
        double Xw[3] = {0.0, 0.0, 0.0};
        for (unsigned i = 0; i + 1 < kTriCandidates; ++i) {
            for (unsigned j = i + 1; j < kTriCandidates; ++j) {
                const bool act = reason == kTriPoint && j < ncand && !(have && best == U);
                if (!__any(act)) continue;                                       // wave-uniform
                const unsigned si = cand_u(cslot, i), sj = cand_u(cslot, j);
                double w[kTriTerms];
#pragma unroll
                for (int k = 0; k < kTriTerms; ++k) {
                    const double wi = cand_d(k, i), wj = cand_d(k, j);
                    double s = 0.0;
                    s = si == walk.l ? s + wi : s;
                    s = sj == walk.l ? s + wj : s;
                    w[k] = combine(s);
                }
                double X[3];
                const bool ok = tri_solve(w, X) && act;
                unsigned score = 0;
                for (unsigned ch = 0; __any(ok && ch < nch); ++ch) {
                    uint64_t pos;
                    bool in;
                    TriObs o = {};
                    TriRay r = {};
                    double e2;
                    const bool usable = fetch(ch, ok && ch < nch, pos, in, o, r);
                    score += (unsigned)__popc(group_bits(usable && tri_inlier(o, X, thr2, e2), walk.base));
                }
                if (ok && (!have || score > best)) {
                    have = true;
                    best = score;
                    pair = i << 16 | j;
#pragma unroll
                    for (int k = 0; k < 3; ++k) Xw[k] = X[k];
                }
            }
        }
        if (reason == kTriPoint) reason = !have ? kTriSingularSystem : best < 2 ? kTriFewInliers : kTriPoint;

        // step 6: least squares over the winner's inliers, then the trimming rounds
        double Xp[3], X[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) Xp[k] = X[k] = Xw[k];
        bool settled = false;
        for (unsigned r = 0; r <= rounds; ++r) {
            const bool act = alive && reason == kTriPoint && !settled;
            if (!__any(act)) break;                                              // wave-uniform
            double acc[kTriTerms];
#pragma unroll
            for (int k = 0; k < kTriTerms; ++k) acc[k] = 0.0;
            unsigned n = 0;
            bool diff = false;
            for (unsigned ch = 0; __any(act && ch < nch); ++ch) {
                uint64_t pos;
                bool in;
                TriObs o = {};
                TriRay ray = {};
                double e2;
                const bool usable = fetch(ch, act && ch < nch, pos, in, o, ray);
                const bool was = usable && tri_inlier(o, Xp, thr2, e2), is = usable && tri_inlier(o, X, thr2, e2);
                if (is) {
                    double w[kTriTerms];
                    tri_contribution(ray, w);
#pragma unroll
                    for (int k = 0; k < kTriTerms; ++k) acc[k] = acc[k] + w[k];
                }
                n += (unsigned)__popc(group_bits(is, walk.base));
                diff = diff || group_bits(was != is, walk.base) != 0;
            }
            double w[kTriTerms], Xn[3];
#pragma unroll
            for (int k = 0; k < kTriTerms; ++k) w[k] = combine(acc[k]);
            const bool ok = tri_solve(w, Xn);
            if (act) {
                if (r > 0 && !diff) settled = true;
                else if (n < 2) reason = kTriFewInliers;
                else if (!ok) reason = kTriSingularSystem;
                else {
#pragma unroll
                    for (int k = 0; k < 3; ++k) Xp[k] = X[k], X[k] = Xn[k];
                }
            }
        }

        // the inliers of the final X: their number, their squared errors' canonical sum and maximum, the first of them
        unsigned n_in = 0;
        double e_sum = 0.0, e_max = 0.0;
        uint64_t first = ~0ull;
        {
            const bool act = alive && reason == kTriPoint;
            for (unsigned ch = 0; __any(act && ch < nch); ++ch) {
                uint64_t pos;
                bool in;
                TriObs o = {};
                TriRay ray = {};
                double e2 = 0.0;
                const bool is = fetch(ch, act && ch < nch, pos, in, o, ray) && tri_inlier(o, X, thr2, e2);
                const unsigned m = group_bits(is, walk.base);
                if (m && first == ~0ull) first = lo + (uint64_t)ch * G + ((unsigned)__ffs((int)m) - 1u);
                n_in += (unsigned)__popc(m);
                e_sum = is ? e_sum + e2 : e_sum;
                e_max = is && e2 > e_max ? e2 : e_max;
            }
            e_sum = combine(e_sum);
#pragma unroll
            for (int m = G / 2; m >= 1; m >>= 1) {
                const double other = __shfl_xor(e_max, m, 64);
                e_max = other > e_max ? other : e_max;
            }
            if (act && n_in < 2) reason = kTriFewInliers;
        }
        const bool point = alive && reason == kTriPoint;

        // step 7: the inlier farthest in angle from the first, then the smallest cosine against that one; the second sweep
        // also writes the states (and is the only one for a track without a point)
        double cosine = 2.0;
        uint64_t anchor = first;
        for (int sweep = 0; sweep < 2; ++sweep) {
            const bool act = sweep == 0 ? point : alive && (point || obs_state != nullptr);
            if (!__any(act)) continue;                                           // wave-uniform
            TriObs oa = {};
            TriRay ra = {};
            if (point && load_obs(tb, poses, anchor, oa)) tri_ray(oa, ra);
            double v = 4.0;
            uint64_t at = ~0ull;
            for (unsigned ch = 0; __any(act && ch < nch); ++ch) {
                uint64_t pos;
                bool in;
                TriObs o = {};
                TriRay ray = {};
                double e2;
                const bool usable = fetch(ch, act && ch < nch, pos, in, o, ray);
                const bool is = point && usable && tri_inlier(o, X, thr2, e2);
                if (is) {
                    const double c = tri_cosine(ra.u, ray.u);
                    if (tri_before(c, pos, v, at)) v = c, at = pos;
                }
                if (sweep == 1 && in && obs_state) obs_state[pos] = is ? 2u : usable ? 1u : 0u;
            }
#pragma unroll
            for (int m = G / 2; m >= 1; m >>= 1) {
                const double ov = __shfl_xor(v, m, 64);
                const uint64_t oat = __shfl_xor((unsigned long long)at, m, 64);
                if (tri_before(ov, oat, v, at)) v = ov, at = oat;
            }
            anchor = at;
            cosine = v;
        }

        if (alive && walk.l == 0) {
            float *p = points + 4 * t;
            unsigned *st = stats + 4 * t;
            p[0] = point ? float(X[0]) : 0.f;
            p[1] = point ? float(X[1]) : 0.f;
            p[2] = point ? float(X[2]) : 0.f;
            p[3] = point ? float(cosine) : 2.f;
            st[0] = U;
            st[1] = point ? n_in : 0u;
            st[2] = reason;
            st[3] = pair;
            if (err) {
                err[2 * t] = point ? float(sqrt(e_sum / double(n_in))) : 0.f;
                err[2 * t + 1] = point ? float(sqrt(e_max)) : 0.f;
            }
        }
    }
}

void launch_triangulate_tracks(const SceneTables &tb, const float *poses, double thr2, unsigned rounds, float *points, unsigned *stats,
                               float *err, unsigned *obs_state, hipStream_t stream) {
    if (tb.tcap == 0) return;
    const uint64_t want = (tb.tcap * G + kThreads - 1) / kThreads;
    hipLaunchKernelGGL(triangulate_tracks, dim3((unsigned)(want < kMaxBlocks ? want : kMaxBlocks)), dim3(kThreads), 0, stream, tb,
                       poses, thr2, rounds, points, stats, err, obs_state);
}

}  // namespace lfmkd
