// Host twin of lf_mkd_bundle_adjust_intrinsics_device (local-features_amd/csrc/mkd_bundle.hip in its double-intrinsics form):
// the kernels' own arithmetic (csrc/mkd_bundle_math.h, compiled here by a plain C++ compiler with -ffp-contract=off) under a
// serial restatement of what the kernels do with it, as tests/cpp/bundle_twin.cpp restates the fixed-intrinsics call -- and
// beside it the groups: which are free, the per-image shares of a group's sums (slot k mod 256 over the image's list), the
// per-group sums of those shares (slot = image id mod 256), the held groups, the two extra terms of the operator, the
// groups' part of the dot products (the sum over the image ids plus the sum over the group ids), the candidate and its
// validity, the rounded intrinsics.  No arithmetic of its own.  tests/bundle_intr_twin.py drives it:
//
//   bundle_intr_twin IN OUT      IN = calls back to back, OUT = their results back to back
//
//   a call: u32 n_images, iterations, cg_iterations, has (1: obs_state, 2: camera_fixed, 4: camera_group), fill, dump, n_groups,
//       refine; f32 max_reproj_px, lambda0, cg_tol, 0; u64 n_rows, track_capacity, obs_capacity; u32 counts[2]; f32
//       kps[n_rows][5]; u64 image_offsets[n_images + 1], track_offsets[track_capacity + 1]; i32 obs_row[obs_capacity]; u32
//       obs_image[obs_capacity]; f32 points[track_capacity][4], intrinsics[n_images][4], poses[n_images][12]; u32
//       obs_state[obs_capacity], camera_fixed[n_images] and camera_group[n_images] where `has` says so
//   ->  u32 poses_out[n_images][12], points_out[track_capacity][4], intrinsics_out[n_images][4], group_out[n_groups][3],
//       obs_state_out[obs_capacity] (every word `fill` where the call writes nothing); f64 trace[iterations][9]; u32 counts[5];
//       with dump != 0 then f64 x[n_images][6] and xg[n_groups][3], the first iteration's camera and group steps
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "mkd_bundle_math.h"

using namespace lfmkd;

namespace {

template <typename T>
void get(FILE *f, T *p, size_t n) {
    if (n && fread(p, sizeof(T), n, f) != n) {
        fprintf(stderr, "bundle_intr_twin: input ends early\n");
        exit(2);
    }
}
template <typename T>
void put(FILE *f, const T *p, size_t n) {
    if (n && fwrite(p, sizeof(T), n, f) != n) {
        fprintf(stderr, "bundle_intr_twin: cannot write\n");
        exit(2);
    }
}

struct Call {
    unsigned n_images, iterations, cg_iterations, has, fill, dump, n_groups, refine, counts[2];
    float px, lambda0, cg_tol;
    uint64_t n_rows, tcap, ocap;
    std::vector<float> kps, points, intr, poses;
    std::vector<uint64_t> ioff, toff;
    std::vector<int> obs_row;
    std::vector<unsigned> obs_image, obs_state, fixed, group;
};

uint64_t clamp_to(uint64_t v, uint64_t total) { return v < total ? v : total; }

// the 4-slot sum of N values over the positions [lo, hi) of a track
template <int N, typename Value>
void track_sum(uint64_t lo, uint64_t hi, Value value, double *out) {
    double slot[N][kTriSlots];
    for (int i = 0; i < N; ++i)
        for (int j = 0; j < kTriSlots; ++j) slot[i][j] = 0.0;
    for (uint64_t p = lo; p < hi; ++p) {
        double w[N];
        if (!value(p, w)) continue;
        for (int i = 0; i < N; ++i) slot[i][(p - lo) % kTriSlots] = slot[i][(p - lo) % kTriSlots] + w[i];
    }
    for (int i = 0; i < N; ++i) out[i] = tri_combine(slot[i]);
}
// the 256-slot sum of N values over M entries
template <int N, typename Value>
void block_sum(uint64_t M, Value value, double *out) {
    static double slot[N][kRsSlots];
    for (int i = 0; i < N; ++i)
        for (int j = 0; j < kRsSlots; ++j) slot[i][j] = 0.0;
    for (uint64_t k = 0; k < M; ++k) {
        double w[N];
        if (!value(k, w)) continue;
        for (int i = 0; i < N; ++i) slot[i][k % kRsSlots] = slot[i][k % kRsSlots] + w[i];
    }
    for (int i = 0; i < N; ++i) out[i] = rs_combine(slot[i]);
}

void run(const Call &q, FILE *out) {
    const unsigned N = q.n_images;
    const double thr2 = double(q.px) * double(q.px), tol2 = double(q.cg_tol) * double(q.cg_tol);
    const unsigned NG = q.n_groups;
    std::vector<unsigned> poses_out(12 * size_t(N), q.fill), points_out(4 * q.tcap, q.fill), state_out(q.ocap, q.fill), counts(5, q.fill);
    std::vector<unsigned> intr_out(4 * size_t(N), q.fill), group_out(3 * size_t(NG), q.fill);
    std::vector<double> trace(size_t(kBaTraceI) * q.iterations, 0.0), dump(q.dump ? 6 * size_t(N) : 0, 0.0),
        dump_g(q.dump ? 3 * size_t(NG) : 0, 0.0);
    if (N == 0) {
        // (the call writes nothing at all: the trace too keeps its fill, which for f64 is the fill word twice)
        std::vector<unsigned> tr(2 * trace.size(), q.fill);
        put(out, poses_out.data(), poses_out.size());
        put(out, points_out.data(), points_out.size());
        put(out, intr_out.data(), intr_out.size());
        put(out, group_out.data(), group_out.size());
        put(out, state_out.data(), state_out.size());
        put(out, tr.data(), tr.size());
        put(out, counts.data(), counts.size());
        return;
    }
    const uint64_t T = clamp_to(q.counts[0], q.tcap), O = clamp_to(q.counts[1], q.ocap);
    const auto K0 = [&](unsigned img) { return &q.intr[4 * size_t(img)]; };
    const auto group_of = [&](unsigned img) { return (q.has & 4) ? q.group[img] : 0u; };
    const auto image_range = [&](unsigned img, uint64_t &lo, uint64_t &hi) {
        lo = clamp_to(q.ioff[img], q.n_rows);
        hi = clamp_to(q.ioff[img + 1], q.n_rows);
        hi = hi > lo ? hi : lo;
    };
    const auto track_range = [&](uint64_t t, uint64_t &lo, uint64_t &hi) {
        lo = clamp_to(q.toff[t], O);
        hi = clamp_to(q.toff[t + 1], O);
        hi = hi > lo ? hi : lo;
    };

    // ba_init
    std::vector<unsigned> head(2 * size_t(N), 0), oflag(q.ocap, 0), tflag(q.tcap, 0), idx(q.n_rows, 0);
    std::vector<unsigned long long> rowmap(q.n_rows, kBaNoRow);
    std::vector<RsPose> cam[2] = {std::vector<RsPose>(N), std::vector<RsPose>(N)};
    std::vector<double> pt[2] = {std::vector<double>(3 * q.tcap, 0.0), std::vector<double>(3 * q.tcap, 0.0)};
    unsigned cur = 0, free_cams = 0, free_points = 0, n_active = 0, accepted = 0, free_groups = 0;
    std::vector<unsigned> gflag(NG, 0);
    std::vector<BaGroup> gstate[2] = {std::vector<BaGroup>(NG, BaGroup{1.0, 0.0, 0.0}), std::vector<BaGroup>(NG, BaGroup{1.0, 0.0, 0.0})};
    const auto group_free = [&](unsigned g) { return g < NG && (gflag[g] & kBaGroupFree); };
    const auto group_moves = [&](unsigned g) { return g < NG && (gflag[g] & (kBaGroupFree | kBaGroupHeld)) == kBaGroupFree; };
    // load_k: the intrinsics image `img` is read under at the groups' state `st`
    struct Kd {
        double v[4];
    };
    const auto K = [&](unsigned st, unsigned img) {
        Kd k;
        ba_widen_k(K0(img), k.v);
        const unsigned g = group_of(img);
        if (group_free(g)) ba_group_k(K0(img), gstate[st][g], k.v);
        return k;
    };
    double lambda = double(q.lambda0);
    for (unsigned i = 0; i < N; ++i) {
        const float *P = &q.poses[12 * size_t(i)];
        const bool usable = tri_camera_usable(K0(i), P), is_free = usable && !((q.has & 2) && q.fixed[i] != 0);
        head[2 * i + 1] = (usable ? kBaCamUsable : 0u) | (is_free ? kBaCamFree : 0u);
        for (int k = 0; k < 9; ++k) cam[0][i].R[k] = double(P[k]);
        for (int k = 0; k < 3; ++k) cam[0][i].t[k] = double(P[9 + k]);
        cam[1][i] = cam[0][i];
    }
    // ba_setup_tracks
    for (uint64_t t = 0; t < T; ++t) {
        uint64_t lo, hi;
        track_range(t, lo, hi);
        const float *p = &q.points[4 * t];
        const bool ok = rs_point_usable(p, 1.0);
        unsigned n = 0;
        for (uint64_t pos = lo; pos < hi; ++pos) {
            const int row = q.obs_row[pos];
            const unsigned img = q.obs_image[pos];
            bool act = false;
            if (ok && row >= 0 && uint64_t(row) < q.n_rows && img < N && (head[2 * size_t(img) + 1] & kBaCamUsable) &&
                (!(q.has & 1) || q.obs_state[pos] == 2u)) {
                uint64_t ilo, ihi;
                image_range(img, ilo, ihi);
                const float *k = &q.kps[5 * size_t(row)];
                act = uint64_t(row) >= ilo && uint64_t(row) < ihi && tri_keypoint_usable(k[0], k[1]);
                if (act) rowmap[row] = (unsigned long long)pos | (unsigned long long)t << 32;
            }
            oflag[pos] = act ? kBaActive : 0u;
            n += act;
        }
        tflag[t] = (ok ? kBaPointOk : 0u) | (n ? kBaPointFree : 0u);
        for (int k = 0; k < 3; ++k) pt[0][3 * t + k] = pt[1][3 * t + k] = double(p[k]);
        free_points += n != 0;
        n_active += n;
    }
    // ba_setup_images: a list for every usable image
    for (unsigned i = 0; i < N; ++i) {
        if (!(head[2 * i + 1] & kBaCamUsable)) continue;
        uint64_t lo, hi;
        image_range(i, lo, hi);
        uint64_t base = lo;
        for (uint64_t r = lo; r < hi; ++r)
            if (rowmap[r] != kBaNoRow && q.obs_image[unsigned(rowmap[r])] == i) idx[base++] = unsigned(r);
        head[2 * i] = unsigned(base - lo);
        free_cams += (head[2 * i + 1] & kBaCamFree) != 0;
    }
    // ba_setup_groups
    for (unsigned g = 0; g < NG; ++g) {
        bool found = false;
        for (unsigned i = 0; i < N; ++i) found = found || (group_of(i) == g && (head[2 * i + 1] & kBaCamUsable) && head[2 * i] != 0);
        if (q.refine && found) gflag[g] = kBaGroupFree, ++free_groups;
    }

    std::vector<double> U(size_t(kRsTerms) * N, 0.0), V(kBaPointTerms * q.tcap, 0.0), W(size_t(kBaW) * q.ocap, 0.0), y(3 * q.tcap, 0.0),
        tcost(q.tcap, 0.0), dots(N, 0.0), vec[5], gU(size_t(kBaGroupTerms) * NG, 0.0), gdots(NG, 0.0), gvec[5],
        Uck(size_t(kBaCk) * N, 0.0), ipart(12 * size_t(N), 0.0);
    std::vector<unsigned> icount(N, 0);
    for (auto &v : vec) v.assign(6 * size_t(N), 0.0);
    for (auto &v : gvec) v.assign(3 * size_t(NG), 0.0);
    enum { X = 0, R = 1, Z = 2, P = 3, AP = 4 };
    const auto corr = [&](uint64_t row, const std::vector<double> &pts, uint64_t t) {
        return BaCorr{q.kps[5 * row], q.kps[5 * row + 1], pts[3 * t], pts[3 * t + 1], pts[3 * t + 2]};
    };
    const auto cam_moves = [&](unsigned i) { return (head[2 * size_t(i) + 1] & (kBaCamFree | kBaCamHeld)) == kBaCamFree; };
    const auto point_moves = [&](uint64_t t) { return (tflag[t] & (kBaPointFree | kBaPointHeld)) == kBaPointFree; };
    const auto sum_dots = [&]() {
        double s, sg;
        block_sum<1>(N, [&](uint64_t i, double *w) { w[0] = dots[i]; return true; }, &s);
        block_sum<1>(NG, [&](uint64_t g, double *w) { w[0] = gdots[g]; return true; }, &sg);
        return s + sg;
    };
    // the rows of an active position at the state (load_lin), and what it adds to sum W^T v over its track (add_wt)
    const auto lin_at = [&](uint64_t pos, uint64_t t, BaLin &o) {
        const unsigned img = q.obs_image[pos];
        ba_rows(cam[cur][img], K(cur, img).v, corr(uint64_t(q.obs_row[pos]), pt[cur], t), o);
    };
    const auto add_wt = [&](uint64_t pos, uint64_t t, int which, double *w) {
        w[0] = w[1] = w[2] = 0.0;
        const unsigned of = oflag[pos];
        if (!(of & (kBaCoupled | kBaInlier))) return false;
        const unsigned img = q.obs_image[pos], g = group_of(img);
        const bool kc = (of & kBaInlier) && group_moves(g);
        if (!(of & kBaCoupled) && !kc) return false;
        BaLin o;
        lin_at(pos, t, o);
        if (of & kBaCoupled) {
            double Wc[kBaW], v[3];
            ba_coupling(o, Wc);
            ba_wt_v(Wc, &vec[which][6 * size_t(img)], v);
            for (int k = 0; k < 3; ++k) w[k] = v[k];
        }
        if (kc) {
            BaGRows gr;
            double Wk[kBaWk], v[3];
            ba_group_rows(o, K0(img), q.refine, gr);
            ba_coupling_k(o, gr, Wk);
            ba_wkt_v(Wk, &gvec[which][3 * size_t(g)], v);
            for (int k = 0; k < 3; ++k) w[k] = (of & kBaCoupled) ? w[k] + v[k] : v[k];
        }
        return true;
    };
    const auto sum_costs = [&]() {
        double s;
        block_sum<1>(T, [&](uint64_t t, double *w) { w[0] = tcost[t]; return true; }, &s);
        return s;
    };

    for (unsigned it = 0; it < q.iterations; ++it) {
        unsigned inliers = 0, held_cams = 0, held_points = 0, held_groups = 0;
        bool bad_sigma = false;
        const std::vector<RsPose> &C = cam[cur];
        const std::vector<double> &Xs = pt[cur];
        // ba_track_lin
        for (uint64_t t = 0; t < T; ++t) {
            uint64_t lo, hi;
            track_range(t, lo, hi);
            unsigned n_in = 0;
            double v[kBaPointTerms], cost, yv[3];
            const auto lin = [&](uint64_t pos, BaLin &o) {
                ba_linearise(C[q.obs_image[pos]], K(cur, q.obs_image[pos]).v, corr(uint64_t(q.obs_row[pos]), Xs, t), thr2, o);
            };
            track_sum<kBaPointTerms>(lo, hi, [&](uint64_t pos, double *w) {
                if (!(oflag[pos] & kBaActive)) return false;
                BaLin o;
                lin(pos, o);
                if (!o.inlier) return false;
                ++n_in;
                ba_point_terms(o, w);
                return true;
            }, v);
            track_sum<1>(lo, hi, [&](uint64_t pos, double *w) {
                if (!(oflag[pos] & kBaActive)) return false;
                BaLin o;
                lin(pos, o);
                w[0] = o.inlier ? o.e2 : thr2;
                return true;
            }, &cost);
            ba_damp_v(v, lambda);
            const bool ok = ba_solve_v(v, v + 6, yv);
            const unsigned tf = tflag[t] & (kBaPointOk | kBaPointFree);
            const bool is_free = (tf & kBaPointFree) != 0, held = is_free && (n_in < 2 || !ok);
            tflag[t] = tf | (held ? kBaPointHeld : 0u);
            tcost[t] = cost;
            for (int k = 0; k < kBaPointTerms; ++k) V[kBaPointTerms * t + k] = v[k];
            for (int k = 0; k < 3; ++k) y[3 * t + k] = is_free && !held ? yv[k] : 0.0;
            inliers += n_in;
            held_points += held;
        }
        // ba_image_lin
        for (unsigned i = 0; i < N; ++i) {
            const unsigned hf = head[2 * size_t(i) + 1] & (kBaCamUsable | kBaCamFree);
            const bool is_free = (hf & kBaCamFree) != 0, informs = (hf & kBaCamUsable) && group_free(group_of(i));
            if (!is_free) {
                for (auto &v : vec)
                    for (int k = 0; k < 6; ++k) v[6 * size_t(i) + k] = 0.0;
                dots[i] = 0.0;
                if (!informs) continue;
            }
            const unsigned M = head[2 * size_t(i)];
            uint64_t lo, hi;
            image_range(i, lo, hi);
            const Kd Ki = K(cur, i);
            const auto lin = [&](uint64_t k, BaLin &o, uint64_t &pos, uint64_t &t) {
                const unsigned row = idx[lo + k];
                pos = unsigned(rowmap[row]), t = rowmap[row] >> 32;
                ba_linearise(C[i], Ki.v, corr(row, Xs, t), thr2, o);
            };
            if (informs) {
                double ga[kBaGroupTerms + kBaCk];
                unsigned n_in = 0;
                block_sum<kBaGroupTerms + kBaCk>(M, [&](uint64_t k, double *w) {
                    BaLin o;
                    uint64_t pos, t;
                    lin(k, o, pos, t);
                    if (!o.inlier) return false;
                    BaGRows gr;
                    ba_group_rows(o, K0(i), q.refine, gr);
                    ba_group_terms(o, gr, w);
                    ba_cross(o, gr, w + kBaGroupTerms);
                    ++n_in;
                    return true;
                }, ga);
                for (int k = 0; k < kBaGroupTerms; ++k) ipart[12 * size_t(i) + k] = ga[k];
                for (int k = 0; k < kBaCk; ++k) Uck[size_t(kBaCk) * i + k] = ga[kBaGroupTerms + k];
                icount[i] = n_in;
            }
            double acc[kRsTerms], z[6], s[6], s3[3], r[6], zz[6];
            block_sum<kRsTerms>(is_free ? M : 0, [&](uint64_t k, double *w) {
                BaLin o;
                uint64_t pos, t;
                lin(k, o, pos, t);
                if (!o.inlier) return false;
                rs_gn_products(o.r, w);
                return true;
            }, acc);
            ba_damp_u(acc, lambda);
            const bool held = !ba_solve_u(acc, acc + 21, z) || !is_free;
            if (is_free) {
                head[2 * size_t(i) + 1] = hf | (held ? kBaCamHeld : 0u);
                held_cams += held;
                for (int k = 0; k < kRsTerms; ++k) U[size_t(kRsTerms) * i + k] = acc[k];
            }
            block_sum<3>(M, [&](uint64_t k, double *w) {
                BaLin o;
                uint64_t pos, t;
                lin(k, o, pos, t);
                if (!(informs && o.inlier && point_moves(t))) return false;
                BaGRows gr;
                double Wk[kBaWk];
                ba_group_rows(o, K0(i), q.refine, gr);
                ba_coupling_k(o, gr, Wk);
                ba_wk_y(Wk, &y[3 * t], w);
                return true;
            }, s3);
            if (informs)
                for (int k = 0; k < 3; ++k) ipart[12 * size_t(i) + 9 + k] = s3[k];
            block_sum<6>(M, [&](uint64_t k, double *w) {
                BaLin o;
                uint64_t pos, t;
                lin(k, o, pos, t);
                const bool coupled = !held && o.inlier && point_moves(t);
                oflag[pos] = kBaActive | (coupled ? kBaCoupled : 0u) | (o.inlier ? kBaInlier : 0u);
                if (!coupled) return false;
                ba_coupling(o, &W[kBaW * pos]);
                ba_w_y(&W[kBaW * pos], &y[3 * t], w);
                return true;
            }, s);
            if (!is_free) continue;
            for (int k = 0; k < 6; ++k) r[k] = held ? 0.0 : acc[21 + k] - s[k];
            ba_solve_u(acc, r, zz);
            for (int k = 0; k < 6; ++k) {
                zz[k] = held ? 0.0 : zz[k];
                vec[X][6 * size_t(i) + k] = 0.0, vec[R][6 * size_t(i) + k] = r[k], vec[Z][6 * size_t(i) + k] = zz[k];
                vec[P][6 * size_t(i) + k] = zz[k], vec[AP][6 * size_t(i) + k] = 0.0;
            }
            dots[i] = held ? 0.0 : ba_dot6(r, zz);
        }
        // ba_group_lin
        for (unsigned g = 0; g < NG; ++g) {
            if (!(gflag[g] & kBaGroupFree)) {
                for (auto &v : gvec)
                    for (int k = 0; k < 3; ++k) v[3 * size_t(g) + k] = 0.0;
                gdots[g] = 0.0;
                continue;
            }
            double acc[12], z[3], r[3], zz[3];
            unsigned n_in = 0;
            block_sum<12>(N, [&](uint64_t i, double *w) {
                if (!(group_of(unsigned(i)) == g && (head[2 * i + 1] & kBaCamUsable))) return false;
                for (int k = 0; k < 12; ++k) w[k] = ipart[12 * i + k];
                n_in += icount[i];
                return true;
            }, acc);
            ba_group_block(acc, lambda, q.refine);
            const bool held = !ba_solve_v(acc, acc + 6, z) || n_in == 0;
            gflag[g] = kBaGroupFree | (held ? kBaGroupHeld : 0u);
            held_groups += held;
            for (int k = 0; k < kBaGroupTerms; ++k) gU[size_t(kBaGroupTerms) * g + k] = acc[k];
            for (int k = 0; k < 3; ++k) r[k] = held ? 0.0 : acc[6 + k] - acc[9 + k];
            ba_group_mask(r, q.refine);
            ba_solve_v(acc, r, zz);
            for (int k = 0; k < 3; ++k) {
                zz[k] = held ? 0.0 : zz[k];
                gvec[X][3 * size_t(g) + k] = 0.0, gvec[R][3 * size_t(g) + k] = r[k], gvec[Z][3 * size_t(g) + k] = zz[k];
                gvec[P][3 * size_t(g) + k] = zz[k], gvec[AP][3 * size_t(g) + k] = 0.0;
            }
            gdots[g] = held ? 0.0 : ba_dot3(r, zz);
        }
        // ba_scalar, start
        const double cost_k = sum_costs();
        BaCg cg;
        ba_cg_start(cg, sum_dots());
        for (unsigned step = 0; step < q.cg_iterations; ++step) {
            if (cg.stopped) break;            // (the kernels are launched and do nothing)
            // ba_track_apply
            for (uint64_t t = 0; t < T; ++t) {
                if (!point_moves(t)) continue;
                uint64_t lo, hi;
                track_range(t, lo, hi);
                double b[3];
                track_sum<3>(lo, hi, [&](uint64_t pos, double *w) { return add_wt(pos, t, P, w); }, b);
                ba_solve_v(&V[kBaPointTerms * t], b, &y[3 * t]);
            }
            // ba_image_apply
            for (unsigned i = 0; i < N; ++i) {
                const unsigned g = group_of(i);
                const bool moves = cam_moves(i), gmoves = (head[2 * size_t(i) + 1] & kBaCamUsable) && group_moves(g);
                if (!moves) {
                    dots[i] = 0.0;
                    if (!gmoves) continue;
                }
                uint64_t lo, hi;
                image_range(i, lo, hi);
                double s[6], s3[3], up[6];
                block_sum<6>(head[2 * size_t(i)], [&](uint64_t k, double *w) {
                    const unsigned long long m = rowmap[idx[lo + k]];
                    if (!(oflag[unsigned(m)] & kBaCoupled)) return false;
                    ba_w_y(&W[kBaW * uint64_t(unsigned(m))], &y[3 * (m >> 32)], w);
                    return true;
                }, s);
                block_sum<3>(head[2 * size_t(i)], [&](uint64_t k, double *w) {
                    const unsigned long long m = rowmap[idx[lo + k]];
                    const uint64_t pos = unsigned(m), t = m >> 32;
                    if (!(gmoves && (oflag[pos] & kBaInlier) && point_moves(t))) return false;
                    BaLin o;
                    BaGRows gr;
                    double Wk[kBaWk];
                    lin_at(pos, t, o);
                    ba_group_rows(o, K0(i), q.refine, gr);
                    ba_coupling_k(o, gr, Wk);
                    ba_wk_y(Wk, &y[3 * t], w);
                    return true;
                }, s3);
                if (moves) {
                    ba_u_times(&U[size_t(kRsTerms) * i], &vec[P][6 * size_t(i)], up);
                    if (gmoves) {
                        double ck[6];
                        ba_w_y(&Uck[size_t(kBaCk) * i], &gvec[P][3 * size_t(g)], ck);
                        for (int k = 0; k < 6; ++k) up[k] = up[k] + ck[k];
                    }
                    for (int k = 0; k < 6; ++k) vec[AP][6 * size_t(i) + k] = up[k] - s[k];
                    dots[i] = ba_dot6(&vec[P][6 * size_t(i)], &vec[AP][6 * size_t(i)]);
                }
                if (gmoves) {
                    double part[3] = {0.0, 0.0, 0.0};
                    if (moves) ba_wt_v(&Uck[size_t(kBaCk) * i], &vec[P][6 * size_t(i)], part);
                    for (int k = 0; k < 3; ++k) ipart[12 * size_t(i) + k] = part[k] - s3[k];
                }
            }
            // ba_group_apply
            for (unsigned g = 0; g < NG; ++g) {
                if (!group_moves(g)) {
                    gdots[g] = 0.0;
                    continue;
                }
                double s[3], up[3], ap[3];
                block_sum<3>(N, [&](uint64_t i, double *w) {
                    if (!(group_of(unsigned(i)) == g && (head[2 * i + 1] & kBaCamUsable))) return false;
                    for (int k = 0; k < 3; ++k) w[k] = ipart[12 * i + k];
                    return true;
                }, s);
                ba_v_times(&gU[size_t(kBaGroupTerms) * g], &gvec[P][3 * size_t(g)], up);
                for (int k = 0; k < 3; ++k) ap[k] = up[k] + s[k];
                ba_group_mask(ap, q.refine);
                for (int k = 0; k < 3; ++k) gvec[AP][3 * size_t(g) + k] = ap[k];
                gdots[g] = ba_dot3(&gvec[P][3 * size_t(g)], ap);
            }
            ba_cg_alpha(cg, sum_dots());
            if (cg.stopped) break;
            // ba_cg_update
            for (unsigned i = 0; i < N; ++i) {
                if (!cam_moves(i)) {
                    dots[i] = 0.0;
                    continue;
                }
                double rn[6], z[6];
                for (int k = 0; k < 6; ++k) {
                    vec[X][6 * size_t(i) + k] = vec[X][6 * size_t(i) + k] + cg.alpha * vec[P][6 * size_t(i) + k];
                    rn[k] = vec[R][6 * size_t(i) + k] - cg.alpha * vec[AP][6 * size_t(i) + k];
                    vec[R][6 * size_t(i) + k] = rn[k];
                }
                ba_solve_u(&U[size_t(kRsTerms) * i], rn, z);
                for (int k = 0; k < 6; ++k) vec[Z][6 * size_t(i) + k] = z[k];
                dots[i] = ba_dot6(rn, z);
            }
            for (unsigned g = 0; g < NG; ++g) {
                if (!group_moves(g)) {
                    gdots[g] = 0.0;
                    continue;
                }
                double rn[3], z[3];
                for (int k = 0; k < 3; ++k) {
                    gvec[X][3 * size_t(g) + k] = gvec[X][3 * size_t(g) + k] + cg.alpha * gvec[P][3 * size_t(g) + k];
                    rn[k] = gvec[R][3 * size_t(g) + k] - cg.alpha * gvec[AP][3 * size_t(g) + k];
                    gvec[R][3 * size_t(g) + k] = rn[k];
                }
                ba_solve_v(&gU[size_t(kBaGroupTerms) * g], rn, z);
                for (int k = 0; k < 3; ++k) gvec[Z][3 * size_t(g) + k] = z[k];
                gdots[g] = ba_dot3(rn, z);
            }
            ba_cg_beta(cg, sum_dots(), tol2);
            if (!cg.stopped) {
                for (size_t k = 0; k < 6 * size_t(N); ++k) vec[P][k] = vec[Z][k] + cg.beta * vec[P][k];
                for (size_t k = 0; k < 3 * size_t(NG); ++k) gvec[P][k] = gvec[Z][k] + cg.beta * gvec[P][k];
            }
        }
        if (q.dump && it == 0) dump = vec[X], dump_g = gvec[X];
        // ba_cam_step
        std::vector<RsPose> &Cn = cam[cur ^ 1];
        std::vector<double> &Xn = pt[cur ^ 1];
        for (unsigned i = 0; i < N; ++i) {
            Cn[i] = C[i];
            if (cam_moves(i)) {
                double d[6];
                for (int k = 0; k < 6; ++k) d[k] = vec[X][6 * size_t(i) + k];
                rs_update(C[i], d, Cn[i]);
            }
        }
        for (unsigned g = 0; g < NG; ++g) {
            gstate[cur ^ 1][g] = gstate[cur][g];
            if (group_moves(g) && !ba_group_step(gstate[cur][g], &gvec[X][3 * size_t(g)], q.refine, gstate[cur ^ 1][g])) bad_sigma = true;
        }
        // ba_track_step
        for (uint64_t t = 0; t < T; ++t) {
            uint64_t lo, hi;
            track_range(t, lo, hi);
            double c[3] = {Xs[3 * t], Xs[3 * t + 1], Xs[3 * t + 2]};
            if (point_moves(t)) {
                double b[3], dp[3];
                track_sum<3>(lo, hi, [&](uint64_t pos, double *w) { return add_wt(pos, t, X, w); }, b);
                for (int k = 0; k < 3; ++k) b[k] = V[kBaPointTerms * t + 6 + k] - b[k];
                ba_solve_v(&V[kBaPointTerms * t], b, dp);
                for (int k = 0; k < 3; ++k) c[k] = c[k] - dp[k];
            }
            for (int k = 0; k < 3; ++k) Xn[3 * t + k] = c[k];
            track_sum<1>(lo, hi, [&](uint64_t pos, double *w) {
                if (!(oflag[pos] & kBaActive)) return false;
                w[0] = rs_cost(Cn[q.obs_image[pos]], K(cur ^ 1, q.obs_image[pos]).v, corr(uint64_t(q.obs_row[pos]), Xn, t), thr2);
                return true;
            }, &tcost[t]);
        }
        // ba_scalar, accept
        const double cost_new = sum_costs(), used = lambda;
        const bool ok = ba_accept(cost_new, cost_k, lambda, !bad_sigma);
        double *row = &trace[size_t(kBaTraceI) * it];
        row[0] = cost_k, row[1] = cost_new, row[2] = used, row[3] = ok ? 1.0 : 0.0, row[4] = double(cg.steps);
        row[5] = double(inliers), row[6] = double(held_cams), row[7] = double(held_points), row[8] = double(held_groups);
        if (ok) cur ^= 1u, ++accepted;
    }

    // ba_final_images, ba_final_tracks
    std::vector<float> rounded(12 * size_t(N));
    for (unsigned i = 0; i < N; ++i) {
        memcpy(&rounded[12 * size_t(i)], &q.poses[12 * size_t(i)], 48);
        if (head[2 * size_t(i) + 1] & kBaCamFree) ba_round_pose(cam[cur][i], &rounded[12 * size_t(i)]);
    }
    memcpy(poses_out.data(), rounded.data(), 48 * size_t(N));
    std::vector<float> Kr(4 * size_t(N));
    for (unsigned i = 0; i < N; ++i) {
        memcpy(&Kr[4 * size_t(i)], K0(i), 16);
        if (group_free(group_of(i))) ba_round_k(K0(i), gstate[cur][group_of(i)], &Kr[4 * size_t(i)]);
    }
    memcpy(intr_out.data(), Kr.data(), 16 * size_t(N));
    for (unsigned g = 0; g < NG; ++g) {
        const float v[3] = {float(gstate[cur][g].s), float(gstate[cur][g].dx), float(gstate[cur][g].dy)};
        memcpy(&group_out[3 * size_t(g)], v, 12);
    }
    for (uint64_t t = 0; t < T; ++t) {
        float p[4];
        memcpy(p, &q.points[4 * t], 16);
        if (tflag[t] & kBaPointFree)
            for (int k = 0; k < 3; ++k) p[k] = float(pt[cur][3 * t + k]);
        memcpy(&points_out[4 * t], p, 16);
        const double Xd[3] = {double(p[0]), double(p[1]), double(p[2])};
        uint64_t lo, hi;
        track_range(t, lo, hi);
        for (uint64_t pos = lo; pos < hi; ++pos) {
            unsigned state = 0;
            if (oflag[pos] & kBaActive) {
                const unsigned img = q.obs_image[pos];
                TriObs o;
                o.x = q.kps[5 * size_t(q.obs_row[pos])], o.y = q.kps[5 * size_t(q.obs_row[pos]) + 1];
                memcpy(o.K, &Kr[4 * size_t(img)], 16);
                memcpy(o.P, &rounded[12 * size_t(img)], 48);
                double e2;
                state = tri_inlier(o, Xd, thr2, e2) ? 2u : 1u;
            }
            state_out[pos] = state;
        }
    }
    counts[0] = free_cams, counts[1] = free_points, counts[2] = n_active, counts[3] = accepted, counts[4] = free_groups;
    put(out, poses_out.data(), poses_out.size());
    put(out, points_out.data(), points_out.size());
    put(out, intr_out.data(), intr_out.size());
    put(out, group_out.data(), group_out.size());
    put(out, state_out.data(), state_out.size());
    put(out, trace.data(), trace.size());
    put(out, counts.data(), counts.size());
    put(out, dump.data(), dump.size());
    put(out, dump_g.data(), dump_g.size());
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: bundle_intr_twin IN OUT\n");
        return 2;
    }
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) {
        fprintf(stderr, "bundle_intr_twin: cannot open %s\n", in ? argv[2] : argv[1]);
        return 2;
    }
    unsigned h[8];
    while (fread(h, sizeof(unsigned), 8, in) == 8) {
        Call q;
        q.n_images = h[0], q.iterations = h[1], q.cg_iterations = h[2], q.has = h[3], q.fill = h[4], q.dump = h[5], q.n_groups = h[6], q.refine = h[7];
        float f[4];
        get(in, f, 4);
        q.px = f[0], q.lambda0 = f[1], q.cg_tol = f[2];
        get(in, &q.n_rows, 1);
        get(in, &q.tcap, 1);
        get(in, &q.ocap, 1);
        get(in, q.counts, 2);
        q.kps.resize(5 * q.n_rows);
        q.ioff.resize(size_t(q.n_images) + 1);
        q.toff.resize(q.tcap + 1);
        q.obs_row.resize(q.ocap);
        q.obs_image.resize(q.ocap);
        q.points.resize(4 * q.tcap);
        q.intr.resize(4 * size_t(q.n_images));
        q.poses.resize(12 * size_t(q.n_images));
        q.obs_state.resize((q.has & 1) ? q.ocap : 0);
        q.fixed.resize((q.has & 2) ? q.n_images : 0);
        q.group.resize((q.has & 4) ? q.n_images : 0);
        get(in, q.kps.data(), q.kps.size());
        get(in, q.ioff.data(), q.ioff.size());
        get(in, q.toff.data(), q.toff.size());
        get(in, q.obs_row.data(), q.obs_row.size());
        get(in, q.obs_image.data(), q.obs_image.size());
        get(in, q.points.data(), q.points.size());
        get(in, q.intr.data(), q.intr.size());
        get(in, q.poses.data(), q.poses.size());
        get(in, q.obs_state.data(), q.obs_state.size());
        get(in, q.fixed.data(), q.fixed.size());
        get(in, q.group.data(), q.group.size());
        run(q, out);
    }
    return fclose(out) == 0 ? 0 : 2;
}
