// C ABI, the geometry: both RANSAC verifiers, two-view poses, track triangulation, camera resection, bundle adjustment,
// view-graph checks.
#include <cmath>
#include <cstring>
#include <vector>

#include "lf_mkd_args.h"
#include "mkd_consts.hpp"
#include "mkd_scene.h"

extern "C" {

// The arguments of both verification entry points.
static int verify_args(lf_mkd *h, bool null_pointer, uint32_t n_hypotheses, float threshold_px, const char *what) {
    const char *msg = nullptr;
    if (null_pointer) msg = "null pointer";
    else if (n_hypotheses == 0 || n_hypotheses > 65536) msg = "n_hypotheses must be 1 .. 65536";
    else if ((msg = threshold_rule(threshold_px))) {}
    else if (!h) msg = "null handle";
    return msg ? refuse(h, what, msg) : LF_MKD_OK;
}

// The device form of both verifiers: the same checks, scratch and grid; `launch` is launch_verify or launch_fundamental.
// Both count one partial per scoring candidate in d_ver_counts: a homography hypothesis has one, a 7-point sample three.
typedef void (*VerifyLaunch)(const float *, const uint64_t *, const float *, const uint64_t *, const int *, unsigned, unsigned,
                             float, unsigned, unsigned, unsigned, VerifyPair *, unsigned *, float *, int *, unsigned *,
                             hipStream_t);
static int verify_device(lf_mkd *h, const lf_mkd_keypoint *d_kps_a, const uint64_t *d_offsets_a, const lf_mkd_keypoint *d_kps_b,
                         const uint64_t *d_offsets_b, const int32_t *d_match, uint32_t n_pairs, uint32_t n_hypotheses,
                         float threshold_px, uint32_t seed, uint32_t flags, float *d_model, int32_t *d_verified,
                         uint32_t *d_stats, void *stream, VerifyLaunch launch, unsigned per_hypothesis, const char *what) {
    const bool null = !d_kps_a || !d_offsets_a || !d_kps_b || !d_offsets_b || !d_match || !d_model || !d_verified || !d_stats;
    if (int rc = verify_args(h, null, n_hypotheses, threshold_px, what)) return rc;
    if (n_pairs == 0) return LF_MKD_OK;
    if (static_cast<const void *>(d_verified) == d_match || static_cast<const void *>(d_verified) == d_kps_a ||
        static_cast<const void *>(d_verified) == d_kps_b)
        return fail(h, LF_MKD_ERR_BAD_ARG, std::string(what) + ": d_verified must not alias d_match or the keypoints");
    // a launch's grid holds fewer than 2^24 workgroups of 256 threads (its work-items are counted in 32 bits)
    const unsigned slices = verify_slices(n_pairs, n_hypotheses, h->num_cus);
    if (uint64_t(n_pairs) * ((n_hypotheses + 255) / 256) * slices >= (1ull << 24))
        return fail(h, LF_MKD_ERR_BAD_ARG, std::string(what) + ": too many pairs x hypotheses for one call (the scoring grid "
                                                               "needs n_pairs x ceil(n_hypotheses / 256) x row slices < 2^24 "
                                                               "workgroups)");
    LF_ENTER(h);
    if (int rc = grow(h, h->d_ver_pairs, n_pairs)) return rc;
    if (int rc = grow(h, h->d_ver_counts, uint64_t(n_pairs) * slices * n_hypotheses * per_hypothesis)) return rc;
    hipStream_t s = stream_of(h, stream);
    launch(reinterpret_cast<const float *>(d_kps_a), d_offsets_a, reinterpret_cast<const float *>(d_kps_b), d_offsets_b, d_match,
           n_pairs, n_hypotheses, threshold_px, seed, flags, slices, h->d_ver_pairs, h->d_ver_counts, d_model, d_verified,
           d_stats, s);
    return launched(h);
}

int lf_mkd_verify_homography_device(lf_mkd *h, const lf_mkd_keypoint *d_kps_a, const uint64_t *d_offsets_a,
                                    const lf_mkd_keypoint *d_kps_b, const uint64_t *d_offsets_b, const int32_t *d_match,
                                    uint32_t n_pairs, uint32_t n_hypotheses, float threshold_px, uint32_t seed, uint32_t flags,
                                    float *d_H, int32_t *d_verified, uint32_t *d_stats, void *stream) {
    return verify_device(h, d_kps_a, d_offsets_a, d_kps_b, d_offsets_b, d_match, n_pairs, n_hypotheses, threshold_px, seed,
                         flags, d_H, d_verified, d_stats, stream, launch_verify, 1, "verify_homography_device");
}

int lf_mkd_verify_fundamental_device(lf_mkd *h, const lf_mkd_keypoint *d_kps_a, const uint64_t *d_offsets_a,
                                     const lf_mkd_keypoint *d_kps_b, const uint64_t *d_offsets_b, const int32_t *d_match,
                                     uint32_t n_pairs, uint32_t n_hypotheses, float threshold_px, uint32_t seed, uint32_t flags,
                                     float *d_F, int32_t *d_verified, uint32_t *d_stats, void *stream) {
    return verify_device(h, d_kps_a, d_offsets_a, d_kps_b, d_offsets_b, d_match, n_pairs, n_hypotheses, threshold_px, seed,
                         flags, d_F, d_verified, d_stats, stream, launch_fundamental, 3, "verify_fundamental_device");
}

// The host form of both verifiers: one pair staged through the handle's d_ver_io, the device form, and the outputs back.
typedef int (*VerifyDevice)(lf_mkd *, const lf_mkd_keypoint *, const uint64_t *, const lf_mkd_keypoint *, const uint64_t *,
                            const int32_t *, uint32_t, uint32_t, float, uint32_t, uint32_t, float *, int32_t *, uint32_t *,
                            void *);
static int verify_host(lf_mkd *h, const lf_mkd_keypoint *kps_a, uint64_t na, const lf_mkd_keypoint *kps_b, uint64_t nb,
                       const int32_t *match, uint32_t n_hypotheses, float threshold_px, uint32_t seed, uint32_t flags,
                       float *model, int32_t *verified, uint32_t *stats, VerifyDevice device, const char *what) {
    const bool null = (na && (!kps_a || !match || !verified)) || (nb && !kps_b) || !model || !stats;
    if (int rc = verify_args(h, null, n_hypotheses, threshold_px, what)) return rc;
    if (above(kRowMax, na, nb)) return fail(h, LF_MKD_ERR_BAD_ARG, std::string(what) + ": more than 2^31 - 1 rows");
    LF_ENTER(h);
    // offsets (a slot of 64 bytes), keypoints of a and b, match, then the outputs: verified, the model (a slot of 48), stats
    Stager io(h, h->d_ver_io);
    const auto d_offs = io.part<uint64_t>(8);
    const auto d_ka = io.part<lf_mkd_keypoint>(na), d_kb = io.part<lf_mkd_keypoint>(nb);
    const auto d_match = io.part<int32_t>(na), d_verified = io.part<int32_t>(na);
    const auto d_model = io.part<float>(12);
    const auto d_stats = io.part<uint32_t>(4);
    if (int rc = io.reserve()) return rc;
    const uint64_t offs[4] = {0, na, 0, nb};
    LF_HIP(h, io.up(d_offs, offs, 4));
    LF_HIP(h, io.up(d_ka, kps_a, na));
    LF_HIP(h, io.up(d_kb, kps_b, nb));
    LF_HIP(h, io.up(d_match, match, na));
    if (int rc = device(h, d_ka, d_offs, d_kb, d_offs.get() + 2, d_match, 1, n_hypotheses, threshold_px, seed, flags, d_model,
                        d_verified, d_stats, h->stream))
        return rc;
    LF_HIP(h, io.down(model, d_model, 9));
    LF_HIP(h, io.down(stats, d_stats, 4));
    LF_HIP(h, io.down(verified, d_verified, na));
    LF_HIP(h, hipStreamSynchronize(h->stream));
    return LF_MKD_OK;
}

int lf_mkd_verify_homography(lf_mkd *h, const lf_mkd_keypoint *kps_a, uint64_t na, const lf_mkd_keypoint *kps_b, uint64_t nb,
                             const int32_t *match, uint32_t n_hypotheses, float threshold_px, uint32_t seed, uint32_t flags,
                             float *H, int32_t *verified, uint32_t *stats) {
    return verify_host(h, kps_a, na, kps_b, nb, match, n_hypotheses, threshold_px, seed, flags, H, verified, stats,
                       lf_mkd_verify_homography_device, "verify_homography");
}

int lf_mkd_verify_fundamental(lf_mkd *h, const lf_mkd_keypoint *kps_a, uint64_t na, const lf_mkd_keypoint *kps_b, uint64_t nb,
                              const int32_t *match, uint32_t n_hypotheses, float threshold_px, uint32_t seed, uint32_t flags,
                              float *F, int32_t *verified, uint32_t *stats) {
    return verify_host(h, kps_a, na, kps_b, nb, match, n_hypotheses, threshold_px, seed, flags, F, verified, stats,
                       lf_mkd_verify_fundamental_device, "verify_fundamental");
}

// Two-view poses (csrc/mkd_two_view_pose.hip).  The cosine of the parallax threshold is formed here, once, in double: no
// transcendental runs on the device (tests/cpp/pose_twin.cpp forms it with the same expression).
static const char *two_view_pose_scalars(float min_parallax_deg, uint32_t flags) {
    if (flags) return "unknown flag bits (no flag is defined: flags must be 0)";
    return parallax_rule(min_parallax_deg);
}

int lf_mkd_two_view_pose_device(lf_mkd *h, const lf_mkd_keypoint *d_kps, uint64_t n_rows_total, const uint32_t *d_edge_a,
                                const uint32_t *d_edge_b, uint32_t n_edges, const float *d_intrinsics, uint32_t n_images,
                                const float *d_F, const uint64_t *d_link_offsets, const int32_t *d_link_a, const int32_t *d_link_b,
                                uint64_t link_capacity, float min_parallax_deg, uint32_t flags, float *d_R, float *d_t,
                                uint32_t *d_stats, float *d_sigma, float *d_points, void *stream) {
    const char *msg = nullptr;
    if (n_edges && (!d_edge_a || !d_edge_b)) msg = "null edge array";
    else if (n_edges && (!d_F || !d_link_offsets || !d_R || !d_t || !d_stats)) msg = "null d_F, d_link_offsets, d_R, d_t or d_stats";
    else if (n_edges && n_images && !d_intrinsics) msg = "null d_intrinsics";
    else if (n_edges && link_capacity && (!d_link_a || !d_link_b)) msg = "null d_link_a or d_link_b";
    else if (n_edges && link_capacity && n_rows_total && !d_kps) msg = "null d_kps";
    else if ((msg = two_view_pose_scalars(min_parallax_deg, flags))) {}
    else if (misaligned(7, d_link_offsets)) msg = "d_link_offsets must be 8-byte aligned";
    else if (misaligned(3, d_kps, d_edge_a, d_edge_b, d_intrinsics, d_F, d_link_a, d_link_b, d_R, d_t, d_stats, d_sigma, d_points))
        msg = "the keypoint, edge, intrinsics, model, link and output arrays must be 4-byte aligned";
    else if (above(kRowMax, n_rows_total, link_capacity, n_edges)) msg = "a total or a capacity above 2^31 - 1";
    else if (!h) msg = "null handle";
    if (msg) return refuse(h, "two_view_pose_device", msg);
    if (n_edges == 0) return LF_MKD_OK;
    LF_ENTER(h);
    const double cmin = std::cos(double(min_parallax_deg) * (3.14159265358979323846 / 180.0));
    launch_two_view_pose(reinterpret_cast<const float *>(d_kps), n_rows_total, d_edge_a, d_edge_b, n_edges, d_intrinsics, n_images,
                         d_F, d_link_offsets, d_link_a, d_link_b, link_capacity, cmin, d_R, d_t, d_stats, d_sigma, d_points,
                         stream_of(h, stream));
    return launched(h);
}

// The host form: one pair.  The pool is a's rows then b's, the two images 0 and 1, the one edge (0, 1); the links are built
// here by the verifiers' rule (row i of a and row match[i] of b iff 0 <= match[i] < nb), staged through the handle's d_ver_io
// with the outputs, and the device call does the rest.  points comes back per row of a: the link's point, or the "none" row.
int lf_mkd_two_view_pose(lf_mkd *h, const float *F, const float *Ka, const float *Kb, const lf_mkd_keypoint *kps_a, uint64_t na,
                         const lf_mkd_keypoint *kps_b, uint64_t nb, const int32_t *match, float min_parallax_deg, uint32_t flags,
                         float *R, float *t, uint32_t *stats, float *sigma, float *points) {
    const char *msg = nullptr;
    if (!F || !Ka || !Kb || !R || !t || !stats) msg = "null pointer";
    else if ((na && (!kps_a || !match)) || (nb && !kps_b)) msg = "null keypoint or match array";
    else if ((msg = two_view_pose_scalars(min_parallax_deg, flags))) {}
    else if (above(kRowMax, na, nb, na + nb)) msg = "more than 2^31 - 1 rows";
    else if (!h) msg = "null handle";
    if (msg) return refuse(h, "two_view_pose", msg);
    LF_ENTER(h);
    std::vector<int32_t> links;   // a's rows, then b's
    for (uint64_t i = 0; i < na; ++i)
        if (match[i] >= 0 && uint64_t(match[i]) < nb) links.push_back(int32_t(i));
    const uint64_t n_links = links.size();
    links.resize(2 * n_links);
    for (uint64_t k = 0; k < n_links; ++k) links[n_links + k] = int32_t(na + uint64_t(match[links[k]]));
    // offsets [2] u64, edge a, edge b, K [2][4], F [9], then the outputs R [9], t [3], stats [4], sigma [3], then the arrays
    Stager io(h, h->d_ver_io);
    const auto d_offs = io.part<uint64_t>(2);
    const auto d_ea = io.part<uint32_t>(1), d_eb = io.part<uint32_t>(1);
    const auto d_K = io.part<float>(8), d_F = io.part<float>(9), d_R = io.part<float>(9), d_t = io.part<float>(3);
    const auto d_stats = io.part<uint32_t>(4);
    const auto d_sigma = io.part<float>(3);
    const auto d_kps = io.part<lf_mkd_keypoint>(na + nb);
    const auto d_la = io.part<int32_t>(n_links), d_lb = io.part<int32_t>(n_links);
    const auto d_points = io.part<float>(points ? 4 * n_links : 0);
    if (int rc = io.reserve()) return rc;
    const uint64_t offs[2] = {0, n_links};
    const uint32_t ea = 0, eb = 1;
    float K[8];
    for (int i = 0; i < 4; ++i) K[i] = Ka[i], K[4 + i] = Kb[i];
    LF_HIP(h, io.up(d_offs, offs, 2));
    LF_HIP(h, io.up(d_ea, &ea, 1));
    LF_HIP(h, io.up(d_eb, &eb, 1));
    LF_HIP(h, io.up(d_K, K, 8));
    LF_HIP(h, io.up(d_F, F, 9));
    LF_HIP(h, io.up(d_kps, kps_a, na));
    LF_HIP(h, io.up(d_kps.get() + na, kps_b, nb));
    LF_HIP(h, io.up(d_la, links.data(), n_links));
    LF_HIP(h, io.up(d_lb, links.data() + n_links, n_links));
    if (int rc = lf_mkd_two_view_pose_device(h, d_kps, na + nb, d_ea, d_eb, 1, d_K, 2, d_F, d_offs, d_la, d_lb, n_links,
                                             min_parallax_deg, flags, d_R, d_t, d_stats, d_sigma, points ? d_points.get() : nullptr,
                                             h->stream))
        return rc;
    std::vector<float> link_points(points ? 4 * n_links : 0);
    LF_HIP(h, io.down(R, d_R, 9));
    LF_HIP(h, io.down(t, d_t, 3));
    LF_HIP(h, io.down(stats, d_stats, 4));
    LF_HIP(h, io.down(sigma, d_sigma, sigma ? 3 : 0));
    LF_HIP(h, io.down(link_points.data(), d_points, link_points.size()));
    LF_HIP(h, hipStreamSynchronize(h->stream));
    if (points) {
        for (uint64_t i = 0; i < na; ++i) points[4 * i] = points[4 * i + 1] = points[4 * i + 2] = 0.f, points[4 * i + 3] = 2.f;
        for (uint64_t k = 0; k < n_links; ++k) std::memcpy(points + 4 * uint64_t(links[k]), link_points.data() + 4 * k, 16);
    }
    return LF_MKD_OK;
}

// Track triangulation (csrc/mkd_triangulate.hip).  The squared threshold is formed here, once, in double
// (tests/cpp/triangulate_twin.cpp forms it with the same expression).
static const char *triangulate_scalars(float max_reproj_px, uint32_t rounds, uint32_t flags) {
    if (flags) return "unknown flag bits (no flag is defined: flags must be 0)";
    if (const char *msg = reproj_rule(max_reproj_px)) return msg;
    return rounds_rule(rounds);
}

int lf_mkd_triangulate_tracks_device(lf_mkd *h, const lf_mkd_keypoint *d_kps, uint64_t n_rows_total, const uint64_t *d_track_offsets,
                                     uint64_t track_capacity, const int32_t *d_obs_row, const uint32_t *d_obs_image,
                                     uint64_t obs_capacity, const uint32_t *d_table_counts, const float *d_intrinsics,
                                     const float *d_poses, uint32_t n_images, float max_reproj_px, uint32_t rounds, uint32_t flags,
                                     float *d_points, uint32_t *d_stats, float *d_err, uint32_t *d_obs_state, void *stream) {
    const char *msg = nullptr;
    if (track_capacity && (!d_track_offsets || !d_table_counts || !d_points || !d_stats))
        msg = "null d_track_offsets, d_table_counts, d_points or d_stats";
    else if (track_capacity && obs_capacity && (!d_obs_row || !d_obs_image)) msg = "null d_obs_row or d_obs_image";
    else if (track_capacity && obs_capacity && n_rows_total && !d_kps) msg = "null d_kps";
    else if (track_capacity && obs_capacity && n_images && (!d_intrinsics || !d_poses)) msg = "null d_intrinsics or d_poses";
    else if ((msg = triangulate_scalars(max_reproj_px, rounds, flags))) {}
    else if (misaligned(7, d_track_offsets)) msg = "d_track_offsets must be 8-byte aligned";
    else if (misaligned(3, d_kps, d_obs_row, d_obs_image, d_table_counts, d_intrinsics, d_poses, d_points, d_stats, d_err, d_obs_state))
        msg = "the keypoint, observation, count, intrinsics, pose and output arrays must be 4-byte aligned";
    else if (above(kRowMax, n_rows_total, track_capacity, obs_capacity)) msg = "a total or a capacity above 2^31 - 1";
    else if (!h) msg = "null handle";
    if (msg) return refuse(h, "triangulate_tracks_device", msg);
    if (track_capacity == 0) return LF_MKD_OK;
    LF_ENTER(h);
    const double thr2 = double(max_reproj_px) * double(max_reproj_px);
    const SceneTables tables = {reinterpret_cast<const float *>(d_kps), n_rows_total, nullptr, n_images, d_track_offsets,
                                track_capacity, d_obs_row, d_obs_image, obs_capacity, d_table_counts, nullptr, d_intrinsics};
    launch_triangulate_tracks(tables, d_poses, thr2, rounds, d_points, d_stats, d_err, d_obs_state, stream_of(h, stream));
    return launched(h);
}

// The host form: the arrays staged through the handle's d_ver_io with the outputs, counts = {n_tracks, n_obs}, and the device
// call does the rest.  obs_state goes up as well as down, so its entries outside every track's range come back as they were.
int lf_mkd_triangulate_tracks(lf_mkd *h, const lf_mkd_keypoint *kps, uint64_t n_rows_total, const uint64_t *track_offsets,
                              uint64_t n_tracks, const int32_t *obs_row, const uint32_t *obs_image, uint64_t n_obs,
                              const float *intrinsics, const float *poses, uint32_t n_images, float max_reproj_px, uint32_t rounds,
                              uint32_t flags, float *points, uint32_t *stats, float *err, uint32_t *obs_state) {
    const char *msg = nullptr;
    if (n_tracks && (!track_offsets || !points || !stats)) msg = "null track_offsets, points or stats";
    else if (n_tracks && n_obs && (!obs_row || !obs_image)) msg = "null obs_row or obs_image";
    else if (n_tracks && n_obs && n_rows_total && !kps) msg = "null kps";
    else if (n_tracks && n_obs && n_images && (!intrinsics || !poses)) msg = "null intrinsics or poses";
    else if ((msg = triangulate_scalars(max_reproj_px, rounds, flags))) {}
    else if (above(kRowMax, n_rows_total, n_tracks, n_obs)) msg = "a total above 2^31 - 1";
    else if (!h) msg = "null handle";
    if (msg) return refuse(h, "triangulate_tracks", msg);
    if (n_tracks == 0) return LF_MKD_OK;
    LF_ENTER(h);
    // counts [2], the arrays in the device call's order, then the outputs
    Stager io(h, h->d_ver_io);
    const auto d_counts = io.part<uint32_t>(2);
    const auto d_offs = io.part<uint64_t>(n_tracks + 1);
    const auto d_kps = io.part<lf_mkd_keypoint>(n_rows_total);
    const auto d_row = io.part<int32_t>(n_obs);
    const auto d_image = io.part<uint32_t>(n_obs);
    const auto d_K = io.part<float>(uint64_t(n_images) * 4), d_poses = io.part<float>(uint64_t(n_images) * 12);
    const auto d_points = io.part<float>(n_tracks * 4);
    const auto d_stats = io.part<uint32_t>(n_tracks * 4);
    const auto d_err = io.part<float>(err ? n_tracks * 2 : 0);
    const auto d_state = io.part<uint32_t>(obs_state ? n_obs : 0);
    if (int rc = io.reserve()) return rc;
    // (counts saturate: the totals are below 2^31)
    const uint32_t counts[2] = {uint32_t(n_tracks), uint32_t(n_obs)};
    LF_HIP(h, io.up(d_counts, counts, 2));
    LF_HIP(h, io.up(d_offs, track_offsets, n_tracks + 1));
    LF_HIP(h, io.up(d_kps, kps, n_obs ? n_rows_total : 0));
    LF_HIP(h, io.up(d_row, obs_row, n_obs));
    LF_HIP(h, io.up(d_image, obs_image, n_obs));
    LF_HIP(h, io.up(d_K, intrinsics, n_obs ? uint64_t(n_images) * 4 : 0));
    LF_HIP(h, io.up(d_poses, poses, n_obs ? uint64_t(n_images) * 12 : 0));
    LF_HIP(h, io.up(d_state, obs_state, obs_state ? n_obs : 0));
    if (int rc = lf_mkd_triangulate_tracks_device(h, d_kps, n_rows_total, d_offs, n_tracks, d_row, d_image, n_obs, d_counts, d_K, d_poses,
                                                  n_images, max_reproj_px, rounds, flags, d_points, d_stats,
                                                  err ? d_err.get() : nullptr, obs_state ? d_state.get() : nullptr, h->stream))
        return rc;
    LF_HIP(h, io.down(points, d_points, n_tracks * 4));
    LF_HIP(h, io.down(stats, d_stats, n_tracks * 4));
    LF_HIP(h, io.down(err, d_err, err ? n_tracks * 2 : 0));
    LF_HIP(h, io.down(obs_state, d_state, obs_state ? n_obs : 0));
    LF_HIP(h, hipStreamSynchronize(h->stream));
    return LF_MKD_OK;
}

// Camera resection (csrc/mkd_resect.hip).  The squared threshold and the parallax cosine are formed here, once, in double
// (tests/cpp/resect_twin.cpp forms them with the same expressions).
static const char *resect_scalars(float max_reproj_px, float min_parallax_deg, uint32_t n_samples, uint32_t rounds, uint32_t flags) {
    if (flags & ~uint32_t(LF_MKD_RESECT_ALL)) return "unknown flag bits";
    if (const char *msg = reproj_rule(max_reproj_px)) return msg;
    if (const char *msg = parallax_rule(min_parallax_deg)) return msg;
    if (n_samples < 1 || n_samples > 4096) return "n_samples must be 1 .. 4096";
    return rounds_rule(rounds);
}

int lf_mkd_resect_cameras_device(lf_mkd *h, const lf_mkd_keypoint *d_kps, const uint64_t *d_image_offsets, uint32_t n_images,
                                 uint64_t n_rows_total, const int32_t *d_row_track, const float *d_points, uint64_t track_capacity,
                                 const uint32_t *d_table_counts, const float *d_intrinsics, const float *d_poses,
                                 float max_reproj_px, float min_parallax_deg, uint32_t n_samples, uint32_t min_inliers,
                                 uint32_t rounds, uint32_t seed, uint32_t flags, float *d_poses_out, uint32_t *d_stats, float *d_err,
                                 uint32_t *d_row_state, void *stream) {
    const char *msg = nullptr;
    if (n_images && (!d_image_offsets || !d_table_counts || !d_intrinsics || !d_poses || !d_poses_out || !d_stats))
        msg = "null d_image_offsets, d_table_counts, d_intrinsics, d_poses, d_poses_out or d_stats";
    else if (n_images && n_rows_total && (!d_kps || !d_row_track)) msg = "null d_kps or d_row_track";
    else if (n_images && n_rows_total && track_capacity && !d_points) msg = "null d_points";
    else if ((msg = resect_scalars(max_reproj_px, min_parallax_deg, n_samples, rounds, flags))) {}
    else if (misaligned(7, d_image_offsets)) msg = "d_image_offsets must be 8-byte aligned";
    else if (misaligned(3, d_kps, d_row_track, d_points, d_table_counts, d_intrinsics, d_poses, d_poses_out, d_stats, d_err, d_row_state))
        msg = "the keypoint, track, point, count, intrinsics, pose and output arrays must be 4-byte aligned";
    else if (above(kRowMax, n_images, n_rows_total, track_capacity))
        msg = "n_images, n_rows_total or track_capacity above 2^31 - 1";
    else if (!h) msg = "null handle";
    if (msg) return refuse(h, "resect_cameras_device", msg);
    if (n_images == 0) return LF_MKD_OK;
    LF_ENTER(h);
    if (int rc = grow(h, h->d_resect, resect_scratch_bytes(n_images, n_rows_total, n_samples))) return rc;
    const double thr2 = double(max_reproj_px) * double(max_reproj_px);
    const double cmin = std::cos(double(min_parallax_deg) * (3.14159265358979323846 / 180.0));
    const SceneTables tables = {reinterpret_cast<const float *>(d_kps), n_rows_total, d_image_offsets, n_images, nullptr,
                                track_capacity, nullptr, nullptr, 0, d_table_counts, d_row_track, d_intrinsics};
    launch_resect_cameras(h->d_resect.get(), tables, d_points, d_poses, thr2, cmin, n_samples, min_inliers, rounds, seed,
                          (flags & LF_MKD_RESECT_ALL) != 0, d_poses_out, d_stats, d_err, d_row_state, stream_of(h, stream));
    return launched(h);
}

// The host form, ONE image: the arrays staged through the handle's d_ver_io with the outputs, offsets = {0, n_rows}, counts =
// {n_tracks}, an all-zero pose, and the device call does the rest.
int lf_mkd_resect_camera(lf_mkd *h, const lf_mkd_keypoint *kps, uint64_t n_rows, const int32_t *row_track, const float *points,
                         uint64_t n_tracks, const float *intrinsics, float max_reproj_px, float min_parallax_deg,
                         uint32_t n_samples, uint32_t min_inliers, uint32_t rounds, uint32_t seed, uint32_t flags, float *pose,
                         uint32_t *stats, float *err, uint32_t *row_state) {
    const char *msg = nullptr;
    if (!intrinsics || !pose || !stats) msg = "null intrinsics, pose or stats";
    else if (n_rows && (!kps || !row_track)) msg = "null kps or row_track";
    else if (n_rows && n_tracks && !points) msg = "null points";
    else if ((msg = resect_scalars(max_reproj_px, min_parallax_deg, n_samples, rounds, flags))) {}
    else if (above(kRowMax, n_rows, n_tracks)) msg = "a total above 2^31 - 1";
    else if (!h) msg = "null handle";
    if (msg) return refuse(h, "resect_camera", msg);
    LF_ENTER(h);
    // offsets [2], counts [2], K [4], the zero pose [12], then the outputs pose [12], stats [4], err [2], then the arrays
    Stager io(h, h->d_ver_io);
    const auto d_offs = io.part<uint64_t>(2);
    const auto d_counts = io.part<uint32_t>(2);
    const auto d_K = io.part<float>(4), d_poses = io.part<float>(12), d_pose = io.part<float>(12);
    const auto d_stats = io.part<uint32_t>(4);
    const auto d_err = io.part<float>(2);
    const auto d_kps = io.part<lf_mkd_keypoint>(n_rows);
    const auto d_track = io.part<int32_t>(n_rows);
    const auto d_points = io.part<float>(n_tracks * 4);
    const auto d_state = io.part<uint32_t>(row_state ? n_rows : 0);
    if (int rc = io.reserve()) return rc;
    const uint64_t offs[2] = {0, n_rows};
    const uint32_t counts[2] = {uint32_t(n_tracks), 0};
    const float zero[12] = {};
    LF_HIP(h, io.up(d_offs, offs, 2));
    LF_HIP(h, io.up(d_counts, counts, 2));
    LF_HIP(h, io.up(d_K, intrinsics, 4));
    LF_HIP(h, io.up(d_poses, zero, 12));
    LF_HIP(h, io.up(d_kps, kps, n_rows));
    LF_HIP(h, io.up(d_track, row_track, n_rows));
    LF_HIP(h, io.up(d_points, points, n_rows ? n_tracks * 4 : 0));
    LF_HIP(h, io.up(d_state, row_state, row_state ? n_rows : 0));
    // (the staged copies are pageable: they have left the host arrays when the calls return)
    if (int rc = lf_mkd_resect_cameras_device(h, d_kps, d_offs, 1, n_rows, d_track, d_points, n_tracks, d_counts, d_K, d_poses,
                                              max_reproj_px, min_parallax_deg, n_samples, min_inliers, rounds, seed, flags, d_pose,
                                              d_stats, d_err, row_state ? d_state.get() : nullptr, h->stream))
        return rc;
    LF_HIP(h, io.down(pose, d_pose, 12));
    LF_HIP(h, io.down(stats, d_stats, 4));
    LF_HIP(h, io.down(err, d_err, err ? 2 : 0));
    LF_HIP(h, io.down(row_state, d_state, row_state ? n_rows : 0));
    LF_HIP(h, hipStreamSynchronize(h->stream));
    return LF_MKD_OK;
}

// Bundle adjustment (csrc/mkd_bundle.hip).  The squared threshold, lambda0 and the squared CG tolerance are formed here, once,
// in double (tests/cpp/bundle_twin.cpp forms them with the same expressions).
static const char *bundle_scalars(float max_reproj_px, float lambda0, uint32_t iterations, uint32_t cg_iterations, float cg_tol,
                                  uint32_t flags) {
    if (flags) return "unknown flag bits (no flag is defined: flags must be 0)";
    if (const char *msg = reproj_rule(max_reproj_px)) return msg;
    if (!(lambda0 > 0.f && std::isfinite(lambda0))) return "lambda0 must be finite and positive";
    if (iterations < 1 || iterations > 64) return "iterations must be 1 .. 64";
    if (cg_iterations < 1 || cg_iterations > 256) return "cg_iterations must be 1 .. 256";
    if (!(cg_tol >= 0.f && cg_tol < 1.f)) return "cg_tol must be in [0, 1)";
    return nullptr;
}

int lf_mkd_bundle_adjust_device(lf_mkd *h, const lf_mkd_keypoint *d_kps, const uint64_t *d_image_offsets, uint32_t n_images,
                                uint64_t n_rows_total, const uint64_t *d_track_offsets, uint64_t track_capacity,
                                const int32_t *d_obs_row, const uint32_t *d_obs_image, uint64_t obs_capacity,
                                const uint32_t *d_table_counts, const float *d_points, const float *d_intrinsics,
                                const float *d_poses, const uint32_t *d_obs_state, const uint32_t *d_camera_fixed,
                                float max_reproj_px, float lambda0, uint32_t iterations, uint32_t cg_iterations, float cg_tol,
                                uint32_t flags, float *d_poses_out, float *d_points_out, uint32_t *d_obs_state_out,
                                double *d_trace, uint32_t *d_counts, void *stream) {
    const char *msg = nullptr;
    if (n_images && (!d_image_offsets || !d_table_counts || !d_intrinsics || !d_poses || !d_poses_out || !d_trace || !d_counts))
        msg = "null d_image_offsets, d_table_counts, d_intrinsics, d_poses, d_poses_out, d_trace or d_counts";
    else if (n_images && track_capacity && (!d_track_offsets || !d_points || !d_points_out))
        msg = "null d_track_offsets, d_points or d_points_out";
    else if (n_images && track_capacity && obs_capacity && (!d_obs_row || !d_obs_image)) msg = "null d_obs_row or d_obs_image";
    else if (n_images && track_capacity && obs_capacity && n_rows_total && !d_kps) msg = "null d_kps";
    else if ((msg = bundle_scalars(max_reproj_px, lambda0, iterations, cg_iterations, cg_tol, flags))) {}
    else if (misaligned(7, d_image_offsets) || misaligned(7, d_track_offsets) || misaligned(7, d_trace))
        msg = "d_image_offsets, d_track_offsets and d_trace must be 8-byte aligned";
    else if (misaligned(3, d_kps, d_obs_row, d_obs_image, d_table_counts, d_points, d_intrinsics, d_poses, d_obs_state, d_camera_fixed,
                        d_poses_out, d_points_out, d_obs_state_out, d_counts))
        msg = "the keypoint, observation, count, point, intrinsics, pose, state, mask and output arrays must be 4-byte aligned";
    else if (above(kRowMax, n_images, n_rows_total, track_capacity, obs_capacity)) msg = "a total or a capacity above 2^31 - 1";
    else if (!h) msg = "null handle";
    if (msg) return refuse(h, "bundle_adjust_device", msg);
    if (n_images == 0) return LF_MKD_OK;
    LF_ENTER(h);
    if (int rc = grow(h, h->d_bundle, bundle_scratch_bytes(n_images, n_rows_total, track_capacity, obs_capacity))) return rc;
    const double thr2 = double(max_reproj_px) * double(max_reproj_px), tol2 = double(cg_tol) * double(cg_tol);
    const SceneTables tables = {reinterpret_cast<const float *>(d_kps), n_rows_total, d_image_offsets, n_images, d_track_offsets,
                                track_capacity, d_obs_row, d_obs_image, obs_capacity, d_table_counts, nullptr, d_intrinsics};
    launch_bundle_adjust(h->d_bundle.get(), tables, d_points, d_poses, d_obs_state, d_camera_fixed, thr2, double(lambda0), iterations,
                         cg_iterations, tol2, d_poses_out, d_points_out, d_obs_state_out, d_trace, d_counts, stream_of(h, stream));
    return launched(h);
}

// The host form: the arrays staged through the handle's d_ver_io with the outputs, counts = {n_tracks, n_obs}, and the device
// call does the rest.  The staged obs_state_out starts as zeros, so its entries outside every track's range come back 0.
int lf_mkd_bundle_adjust(lf_mkd *h, const lf_mkd_keypoint *kps, const uint64_t *image_offsets, uint32_t n_images,
                         uint64_t n_rows_total, const uint64_t *track_offsets, uint64_t n_tracks, const int32_t *obs_row,
                         const uint32_t *obs_image, uint64_t n_obs, const float *points, const float *intrinsics,
                         const float *poses, const uint32_t *obs_state, const uint32_t *camera_fixed, float max_reproj_px,
                         float lambda0, uint32_t iterations, uint32_t cg_iterations, float cg_tol, uint32_t flags,
                         float *poses_out, float *points_out, uint32_t *obs_state_out, double *trace, uint32_t *counts) {
    const char *msg = nullptr;
    if (n_images && (!image_offsets || !intrinsics || !poses || !poses_out || !trace || !counts))
        msg = "null image_offsets, intrinsics, poses, poses_out, trace or counts";
    else if (n_images && n_tracks && (!track_offsets || !points || !points_out)) msg = "null track_offsets, points or points_out";
    else if (n_images && n_tracks && n_obs && (!obs_row || !obs_image)) msg = "null obs_row or obs_image";
    else if (n_images && n_tracks && n_obs && n_rows_total && !kps) msg = "null kps";
    else if ((msg = bundle_scalars(max_reproj_px, lambda0, iterations, cg_iterations, cg_tol, flags))) {}
    else if (above(kRowMax, n_images, n_rows_total, n_tracks, n_obs)) msg = "a total above 2^31 - 1";
    else if (!h) msg = "null handle";
    if (msg) return refuse(h, "bundle_adjust", msg);
    if (n_images == 0) return LF_MKD_OK;
    LF_ENTER(h);
    Stager io(h, h->d_ver_io);
    const auto d_trace = io.part<double>(uint64_t(iterations) * 8);
    const auto d_ioff = io.part<uint64_t>(uint64_t(n_images) + 1), d_toff = io.part<uint64_t>(n_tracks + 1);
    const auto d_tc = io.part<uint32_t>(2), d_counts = io.part<uint32_t>(4);
    const auto d_kps = io.part<lf_mkd_keypoint>(n_rows_total);
    const auto d_row = io.part<int32_t>(n_obs);
    const auto d_image = io.part<uint32_t>(n_obs);
    const auto d_points = io.part<float>(n_tracks * 4), d_K = io.part<float>(uint64_t(n_images) * 4);
    const auto d_poses = io.part<float>(uint64_t(n_images) * 12);
    const auto d_state = io.part<uint32_t>(obs_state ? n_obs : 0), d_fixed = io.part<uint32_t>(camera_fixed ? n_images : 0);
    const auto d_state_out = io.part<uint32_t>(obs_state_out ? n_obs : 0);
    if (int rc = io.reserve()) return rc;
    const uint32_t tc[2] = {uint32_t(n_tracks), uint32_t(n_obs)};
    LF_HIP(h, io.up(d_ioff, image_offsets, uint64_t(n_images) + 1));
    LF_HIP(h, io.up(d_toff, track_offsets, n_tracks ? n_tracks + 1 : 0));
    LF_HIP(h, io.up(d_tc, tc, 2));
    LF_HIP(h, io.up(d_kps, kps, n_tracks && n_obs ? n_rows_total : 0));
    LF_HIP(h, io.up(d_row, obs_row, n_tracks ? n_obs : 0));
    LF_HIP(h, io.up(d_image, obs_image, n_tracks ? n_obs : 0));
    LF_HIP(h, io.up(d_points, points, n_tracks * 4));
    LF_HIP(h, io.up(d_K, intrinsics, uint64_t(n_images) * 4));
    LF_HIP(h, io.up(d_poses, poses, uint64_t(n_images) * 12));
    LF_HIP(h, io.up(d_state, obs_state, obs_state && n_tracks ? n_obs : 0));
    LF_HIP(h, io.up(d_fixed, camera_fixed, camera_fixed ? n_images : 0));
    if (obs_state_out && n_obs) LF_HIP(h, hipMemsetAsync(d_state_out.get(), 0, n_obs * 4, h->stream));
    // (in place on the staged poses and points)
    if (int rc = lf_mkd_bundle_adjust_device(h, d_kps, d_ioff, n_images, n_rows_total, d_toff, n_tracks, d_row, d_image, n_obs, d_tc,
                                             d_points, d_K, d_poses, obs_state ? d_state.get() : nullptr,
                                             camera_fixed ? d_fixed.get() : nullptr, max_reproj_px, lambda0, iterations, cg_iterations,
                                             cg_tol, flags, d_poses, d_points, obs_state_out ? d_state_out.get() : nullptr, d_trace,
                                             d_counts, h->stream))
        return rc;
    LF_HIP(h, io.down(poses_out, d_poses, uint64_t(n_images) * 12));
    LF_HIP(h, io.down(points_out, d_points, n_tracks * 4));
    LF_HIP(h, io.down(obs_state_out, d_state_out, obs_state_out ? n_obs : 0));
    LF_HIP(h, io.down(trace, d_trace, uint64_t(iterations) * 8));
    LF_HIP(h, io.down(counts, d_counts, 4));
    LF_HIP(h, hipStreamSynchronize(h->stream));
    return LF_MKD_OK;
}

// Bundle adjustment with shared intrinsics refined: the same kernels in their double-intrinsics form (csrc/mkd_bundle.hip),
// the same scalars formed the same way (tests/cpp/bundle_intr_twin.cpp).
static const char *bundle_groups(uint32_t n_images, const void *camera_group, uint32_t n_groups, uint32_t refine) {
    if (refine > (LF_MKD_BA_REFINE_FOCAL | LF_MKD_BA_REFINE_PRINCIPAL))
        return "unknown refine bits (LF_MKD_BA_REFINE_FOCAL | LF_MKD_BA_REFINE_PRINCIPAL)";
    if (n_images && n_groups == 0) return "n_groups must be at least 1";
    if (n_images && !camera_group && n_groups != 1) return "a null camera_group puts every image in group 0: n_groups must be 1";
    return nullptr;
}

int lf_mkd_bundle_adjust_intrinsics_device(lf_mkd *h, const lf_mkd_keypoint *d_kps, const uint64_t *d_image_offsets, uint32_t n_images,
                                           uint64_t n_rows_total, const uint64_t *d_track_offsets, uint64_t track_capacity,
                                           const int32_t *d_obs_row, const uint32_t *d_obs_image, uint64_t obs_capacity,
                                           const uint32_t *d_table_counts, const float *d_points, const float *d_intrinsics,
                                           const float *d_poses, const uint32_t *d_obs_state, const uint32_t *d_camera_fixed,
                                           const uint32_t *d_camera_group, uint32_t n_groups, uint32_t refine, float max_reproj_px,
                                           float lambda0, uint32_t iterations, uint32_t cg_iterations, float cg_tol, uint32_t flags,
                                           float *d_poses_out, float *d_points_out, float *d_intrinsics_out, float *d_group_out,
                                           uint32_t *d_obs_state_out, double *d_trace, uint32_t *d_counts, void *stream) {
    const char *msg = nullptr;
    if (n_images && (!d_image_offsets || !d_table_counts || !d_intrinsics || !d_poses || !d_poses_out || !d_intrinsics_out || !d_trace ||
                     !d_counts))
        msg = "null d_image_offsets, d_table_counts, d_intrinsics, d_poses, d_poses_out, d_intrinsics_out, d_trace or d_counts";
    else if (n_images && track_capacity && (!d_track_offsets || !d_points || !d_points_out))
        msg = "null d_track_offsets, d_points or d_points_out";
    else if (n_images && track_capacity && obs_capacity && (!d_obs_row || !d_obs_image)) msg = "null d_obs_row or d_obs_image";
    else if (n_images && track_capacity && obs_capacity && n_rows_total && !d_kps) msg = "null d_kps";
    else if ((msg = bundle_groups(n_images, d_camera_group, n_groups, refine))) {}
    else if ((msg = bundle_scalars(max_reproj_px, lambda0, iterations, cg_iterations, cg_tol, flags))) {}
    else if (misaligned(7, d_image_offsets) || misaligned(7, d_track_offsets) || misaligned(7, d_trace))
        msg = "d_image_offsets, d_track_offsets and d_trace must be 8-byte aligned";
    else if (misaligned(3, d_kps, d_obs_row, d_obs_image, d_table_counts, d_points, d_intrinsics, d_poses, d_obs_state, d_camera_fixed,
                        d_camera_group, d_poses_out, d_points_out, d_intrinsics_out, d_group_out, d_obs_state_out, d_counts))
        msg = "the keypoint, observation, count, point, intrinsics, pose, state, mask, group and output arrays must be 4-byte aligned";
    else if (above(kRowMax, n_images, n_rows_total, track_capacity, obs_capacity, n_groups)) msg = "a total or a capacity above 2^31 - 1";
    else if (!h) msg = "null handle";
    if (msg) return refuse(h, "bundle_adjust_intrinsics_device", msg);
    if (n_images == 0) return LF_MKD_OK;
    LF_ENTER(h);
    if (int rc = grow(h, h->d_bundle, bundle_intrinsics_scratch_bytes(n_images, n_rows_total, track_capacity, obs_capacity, n_groups)))
        return rc;
    const double thr2 = double(max_reproj_px) * double(max_reproj_px), tol2 = double(cg_tol) * double(cg_tol);
    const SceneTables tables = {reinterpret_cast<const float *>(d_kps), n_rows_total, d_image_offsets, n_images, d_track_offsets,
                                track_capacity, d_obs_row, d_obs_image, obs_capacity, d_table_counts, nullptr, d_intrinsics};
    launch_bundle_adjust_intrinsics(h->d_bundle.get(), tables, d_points, d_poses, d_obs_state, d_camera_fixed, d_camera_group, n_groups,
                                    refine, thr2, double(lambda0), iterations, cg_iterations, tol2, d_poses_out, d_points_out,
                                    d_intrinsics_out, d_group_out, d_obs_state_out, d_trace, d_counts, stream_of(h, stream));
    return launched(h);
}

// The host form, staged as lf_mkd_bundle_adjust stages its arrays; in place on the staged poses, points and intrinsics.
int lf_mkd_bundle_adjust_intrinsics(lf_mkd *h, const lf_mkd_keypoint *kps, const uint64_t *image_offsets, uint32_t n_images,
                                    uint64_t n_rows_total, const uint64_t *track_offsets, uint64_t n_tracks, const int32_t *obs_row,
                                    const uint32_t *obs_image, uint64_t n_obs, const float *points, const float *intrinsics,
                                    const float *poses, const uint32_t *obs_state, const uint32_t *camera_fixed,
                                    const uint32_t *camera_group, uint32_t n_groups, uint32_t refine, float max_reproj_px,
                                    float lambda0, uint32_t iterations, uint32_t cg_iterations, float cg_tol, uint32_t flags,
                                    float *poses_out, float *points_out, float *intrinsics_out, float *group_out,
                                    uint32_t *obs_state_out, double *trace, uint32_t *counts) {
    const char *msg = nullptr;
    if (n_images && (!image_offsets || !intrinsics || !poses || !poses_out || !intrinsics_out || !trace || !counts))
        msg = "null image_offsets, intrinsics, poses, poses_out, intrinsics_out, trace or counts";
    else if (n_images && n_tracks && (!track_offsets || !points || !points_out)) msg = "null track_offsets, points or points_out";
    else if (n_images && n_tracks && n_obs && (!obs_row || !obs_image)) msg = "null obs_row or obs_image";
    else if (n_images && n_tracks && n_obs && n_rows_total && !kps) msg = "null kps";
    else if ((msg = bundle_groups(n_images, camera_group, n_groups, refine))) {}
    else if ((msg = bundle_scalars(max_reproj_px, lambda0, iterations, cg_iterations, cg_tol, flags))) {}
    else if (above(kRowMax, n_images, n_rows_total, n_tracks, n_obs, n_groups)) msg = "a total above 2^31 - 1";
    else if (!h) msg = "null handle";
    if (msg) return refuse(h, "bundle_adjust_intrinsics", msg);
    if (n_images == 0) return LF_MKD_OK;
    LF_ENTER(h);
    Stager io(h, h->d_ver_io);
    const auto d_trace = io.part<double>(uint64_t(iterations) * 9);
    const auto d_ioff = io.part<uint64_t>(uint64_t(n_images) + 1), d_toff = io.part<uint64_t>(n_tracks + 1);
    const auto d_tc = io.part<uint32_t>(2), d_counts = io.part<uint32_t>(5);
    const auto d_kps = io.part<lf_mkd_keypoint>(n_rows_total);
    const auto d_row = io.part<int32_t>(n_obs);
    const auto d_image = io.part<uint32_t>(n_obs);
    const auto d_points = io.part<float>(n_tracks * 4), d_K = io.part<float>(uint64_t(n_images) * 4);
    const auto d_poses = io.part<float>(uint64_t(n_images) * 12);
    const auto d_state = io.part<uint32_t>(obs_state ? n_obs : 0), d_fixed = io.part<uint32_t>(camera_fixed ? n_images : 0);
    const auto d_group = io.part<uint32_t>(camera_group ? n_images : 0);
    const auto d_gout = io.part<float>(group_out ? uint64_t(n_groups) * 3 : 0);
    const auto d_state_out = io.part<uint32_t>(obs_state_out ? n_obs : 0);
    if (int rc = io.reserve()) return rc;
    const uint32_t tc[2] = {uint32_t(n_tracks), uint32_t(n_obs)};
    LF_HIP(h, io.up(d_ioff, image_offsets, uint64_t(n_images) + 1));
    LF_HIP(h, io.up(d_toff, track_offsets, n_tracks ? n_tracks + 1 : 0));
    LF_HIP(h, io.up(d_tc, tc, 2));
    LF_HIP(h, io.up(d_kps, kps, n_tracks && n_obs ? n_rows_total : 0));
    LF_HIP(h, io.up(d_row, obs_row, n_tracks ? n_obs : 0));
    LF_HIP(h, io.up(d_image, obs_image, n_tracks ? n_obs : 0));
    LF_HIP(h, io.up(d_points, points, n_tracks * 4));
    LF_HIP(h, io.up(d_K, intrinsics, uint64_t(n_images) * 4));
    LF_HIP(h, io.up(d_poses, poses, uint64_t(n_images) * 12));
    LF_HIP(h, io.up(d_state, obs_state, obs_state && n_tracks ? n_obs : 0));
    LF_HIP(h, io.up(d_fixed, camera_fixed, camera_fixed ? n_images : 0));
    LF_HIP(h, io.up(d_group, camera_group, camera_group ? n_images : 0));
    if (obs_state_out && n_obs) LF_HIP(h, hipMemsetAsync(d_state_out.get(), 0, n_obs * 4, h->stream));
    if (int rc = lf_mkd_bundle_adjust_intrinsics_device(
            h, d_kps, d_ioff, n_images, n_rows_total, d_toff, n_tracks, d_row, d_image, n_obs, d_tc, d_points, d_K, d_poses,
            obs_state ? d_state.get() : nullptr, camera_fixed ? d_fixed.get() : nullptr, camera_group ? d_group.get() : nullptr, n_groups,
            refine, max_reproj_px, lambda0, iterations, cg_iterations, cg_tol, flags, d_poses, d_points, d_K,
            group_out ? d_gout.get() : nullptr, obs_state_out ? d_state_out.get() : nullptr, d_trace, d_counts, h->stream))
        return rc;
    LF_HIP(h, io.down(poses_out, d_poses, uint64_t(n_images) * 12));
    LF_HIP(h, io.down(points_out, d_points, n_tracks * 4));
    LF_HIP(h, io.down(intrinsics_out, d_K, uint64_t(n_images) * 4));
    LF_HIP(h, io.down(group_out, d_gout, group_out ? uint64_t(n_groups) * 3 : 0));
    LF_HIP(h, io.down(obs_state_out, d_state_out, obs_state_out ? n_obs : 0));
    LF_HIP(h, io.down(trace, d_trace, uint64_t(iterations) * 9));
    LF_HIP(h, io.down(counts, d_counts, 5));
    LF_HIP(h, hipStreamSynchronize(h->stream));
    return LF_MKD_OK;
}

// View-graph checks (csrc/mkd_view_graph.hip).  The cosine of the loop threshold is formed here, once, in double: no
// transcendental runs on the device (tests/cpp/view_graph_twin.cpp forms it with the same expression).
static const char *view_graph_scalars(uint32_t n_images, uint32_t n_edges, float max_loop_deg, uint32_t root, uint32_t tree_rounds,
                                      uint32_t iterations, uint32_t flags) {
    if (flags & ~uint32_t(LF_MKD_VIEW_GRAPH_USE_UNCHECKED)) return "unknown flag bits";
    if (!(max_loop_deg >= 0.f && max_loop_deg <= 180.f)) return "max_loop_deg must be in [0, 180]";
    if (n_images && root != LF_MKD_VIEW_GRAPH_AUTO_ROOT && root >= n_images) return "root must be an image id or LF_MKD_VIEW_GRAPH_AUTO_ROOT";
    if (tree_rounds > LF_MKD_VIEW_GRAPH_MAX_ROUNDS || iterations > LF_MKD_VIEW_GRAPH_MAX_ROUNDS)
        return "tree_rounds and iterations must be 0 .. 4096 (each is a launch)";
    if (above(kRowMax, uint64_t(n_images) * n_images)) return "a table of more than 2^31 - 1 entries (n_images^2)";
    if (above(kRowMax, n_edges)) return "n_edges above 2^31 - 1";
    return nullptr;
}

int lf_mkd_view_graph_plan(uint32_t n_images, uint32_t n_edges, uint32_t tree_rounds, uint32_t iterations, uint32_t flags,
                           uint32_t with_match, uint32_t *launches, uint64_t *scratch_bytes, uint32_t *form) {
    if (const char *msg = view_graph_scalars(n_images, n_edges, 0.f, LF_MKD_VIEW_GRAPH_AUTO_ROOT, tree_rounds, iterations, flags))
        return refuse(nullptr, "view_graph_plan", msg);
    const ViewGraphPlan p = view_graph_plan(n_images, n_edges, tree_rounds, iterations, with_match != 0);
    if (launches) *launches = p.launches;
    if (scratch_bytes) *scratch_bytes = p.scratch_bytes;
    if (form) *form = LF_MKD_VIEW_GRAPH_FORM_TABLE;
    return LF_MKD_OK;
}

int lf_mkd_view_graph_device(lf_mkd *h, const uint32_t *d_edge_a, const uint32_t *d_edge_b, uint32_t n_edges, const float *d_R,
                             const uint32_t *d_pose_stats, uint32_t n_images, float max_loop_deg, uint32_t min_front, uint32_t root,
                             uint32_t tree_rounds, uint32_t iterations, uint32_t flags, const uint64_t *d_edge_offsets_a,
                             uint64_t ea_capacity, const int32_t *d_match, int32_t *d_match_out, float *d_rotations,
                             uint32_t *d_edge_stats, float *d_edge_residual, uint32_t *d_image_stats, uint32_t *d_counts,
                             void *stream) {
    const int filter = (d_edge_offsets_a != nullptr) + (d_match != nullptr) + (d_match_out != nullptr);
    const char *msg = nullptr;
    if (n_images && (!d_rotations || !d_image_stats || !d_counts)) msg = "null d_rotations, d_image_stats or d_counts";
    else if (n_images && n_edges && (!d_edge_a || !d_edge_b || !d_R || !d_pose_stats || !d_edge_stats))
        msg = "null d_edge_a, d_edge_b, d_R, d_pose_stats or d_edge_stats";
    else if (filter != 0 && filter != 3) msg = "d_edge_offsets_a, d_match and d_match_out go together (all three, or none)";
    else if ((msg = view_graph_scalars(n_images, n_edges, max_loop_deg, root, tree_rounds, iterations, flags))) {}
    else if (misaligned(7, d_edge_offsets_a)) msg = "d_edge_offsets_a must be 8-byte aligned";
    else if (misaligned(3, d_edge_a, d_edge_b, d_R, d_pose_stats, d_match, d_match_out, d_rotations, d_edge_stats, d_edge_residual,
                        d_image_stats, d_counts))
        msg = "the edge, rotation, statistics, match and output arrays must be 4-byte aligned";
    else if (above(kRowMax, ea_capacity)) msg = "ea_capacity above 2^31 - 1";
    else if (!h) msg = "null handle";
    if (msg) return refuse(h, "view_graph_device", msg);
    if (n_images == 0) return LF_MKD_OK;
    LF_ENTER(h);
    const ViewGraphPlan plan = view_graph_plan(n_images, n_edges, tree_rounds, iterations, filter == 3);
    unsigned char *work;
    if (int rc = scratch(h, h->d_view_graph, plan.scratch_bytes, &work)) return rc;
    const double cmax = std::cos(double(max_loop_deg) * (3.14159265358979323846 / 180.0));
    const unsigned issued =
        launch_view_graph(plan, work, d_edge_a, d_edge_b, n_edges, d_R, d_pose_stats, n_images, cmax, min_front, root, tree_rounds,
                      iterations, (flags & LF_MKD_VIEW_GRAPH_USE_UNCHECKED) != 0, d_edge_offsets_a, ea_capacity, d_match, d_match_out,
                      d_rotations, d_edge_stats, d_edge_residual, d_image_stats, d_counts, stream_of(h, stream));
    if (issued != plan.launches)
        return fail(h, LF_MKD_ERR_HIP, "view_graph_device: issued " + std::to_string(issued) + " launches, the plan says " +
                                           std::to_string(plan.launches));
    return launched(h);
}

// The host form: the arrays staged through the handle's d_ver_io with the outputs, and the device call does the rest.  The
// match array is filtered in place on its staged copy, so match_out's entries outside every edge's range come back as match's.
int lf_mkd_view_graph(lf_mkd *h, const uint32_t *edge_a, const uint32_t *edge_b, uint32_t n_edges, const float *R,
                      const uint32_t *pose_stats, uint32_t n_images, float max_loop_deg, uint32_t min_front, uint32_t root,
                      uint32_t tree_rounds, uint32_t iterations, uint32_t flags, const uint64_t *edge_offsets_a, uint64_t n_entries,
                      const int32_t *match, int32_t *match_out, float *rotations, uint32_t *edge_stats, float *edge_residual,
                      uint32_t *image_stats, uint32_t *counts) {
    const int filter = (edge_offsets_a != nullptr) + (match != nullptr) + (match_out != nullptr);
    const char *msg = nullptr;
    if (n_images && (!rotations || !image_stats || !counts)) msg = "null rotations, image_stats or counts";
    else if (n_images && n_edges && (!edge_a || !edge_b || !R || !pose_stats || !edge_stats))
        msg = "null edge_a, edge_b, R, pose_stats or edge_stats";
    else if (filter != 0 && filter != 3) msg = "edge_offsets_a, match and match_out go together (all three, or none)";
    else if ((msg = view_graph_scalars(n_images, n_edges, max_loop_deg, root, tree_rounds, iterations, flags))) {}
    else if (above(kRowMax, n_entries)) msg = "n_entries above 2^31 - 1";
    else if (!h) msg = "null handle";
    if (msg) return refuse(h, "view_graph", msg);
    if (n_images == 0) return LF_MKD_OK;
    LF_ENTER(h);
    const uint64_t n_match = filter == 3 && n_edges ? n_entries : 0;
    Stager io(h, h->d_ver_io);
    const auto d_off = io.part<uint64_t>(filter == 3 ? uint64_t(n_edges) + 1 : 0);
    const auto d_ea = io.part<uint32_t>(n_edges), d_eb = io.part<uint32_t>(n_edges);
    const auto d_R = io.part<float>(uint64_t(n_edges) * 9);
    const auto d_ps = io.part<uint32_t>(uint64_t(n_edges) * 4);
    const auto d_match = io.part<int32_t>(n_match);
    const auto d_rot = io.part<float>(uint64_t(n_images) * 9);
    const auto d_es = io.part<uint32_t>(uint64_t(n_edges) * 4);
    const auto d_res = io.part<float>(edge_residual ? n_edges : 0);
    const auto d_is = io.part<uint32_t>(uint64_t(n_images) * 4);
    const auto d_counts = io.part<uint32_t>(8);
    if (int rc = io.reserve()) return rc;
    LF_HIP(h, io.up(d_off, edge_offsets_a, filter == 3 ? uint64_t(n_edges) + 1 : 0));
    LF_HIP(h, io.up(d_ea, edge_a, n_edges));
    LF_HIP(h, io.up(d_eb, edge_b, n_edges));
    LF_HIP(h, io.up(d_R, R, uint64_t(n_edges) * 9));
    LF_HIP(h, io.up(d_ps, pose_stats, uint64_t(n_edges) * 4));
    LF_HIP(h, io.up(d_match, match, n_match));
    if (int rc = lf_mkd_view_graph_device(h, d_ea, d_eb, n_edges, d_R, d_ps, n_images, max_loop_deg, min_front, root, tree_rounds,
                                          iterations, flags, filter == 3 ? d_off.get() : nullptr, n_match,
                                          filter == 3 ? d_match.get() : nullptr, filter == 3 ? d_match.get() : nullptr, d_rot, d_es,
                                          edge_residual ? d_res.get() : nullptr, d_is, d_counts, h->stream))
        return rc;
    LF_HIP(h, io.down(rotations, d_rot, uint64_t(n_images) * 9));
    LF_HIP(h, io.down(edge_stats, d_es, uint64_t(n_edges) * 4));
    LF_HIP(h, io.down(edge_residual, d_res, edge_residual ? n_edges : 0));
    LF_HIP(h, io.down(image_stats, d_is, uint64_t(n_images) * 4));
    LF_HIP(h, io.down(counts, d_counts, 8));
    LF_HIP(h, io.down(match_out, d_match, n_match));
    LF_HIP(h, hipStreamSynchronize(h->stream));
    // (without edges there is nothing to filter: match_out is match)
    if (filter == 3 && !n_edges && match_out != match) std::memcpy(match_out, match, n_entries * sizeof(int32_t));
    return LF_MKD_OK;
}

// Tree poses (csrc/mkd_positions.hip): one launch, no scratch.
int lf_mkd_tree_poses_device(lf_mkd *h, const uint32_t *d_edge_a, const uint32_t *d_edge_b, const float *d_t, uint32_t n_edges,
                             const float *d_rotations, const uint32_t *d_image_stats, uint32_t n_images, uint32_t max_depth,
                             float *d_poses, void *stream) {
    const char *msg = nullptr;
    if (n_images && (!d_rotations || !d_image_stats || !d_poses)) msg = "null d_rotations, d_image_stats or d_poses";
    else if (n_images && n_edges && (!d_edge_a || !d_edge_b || !d_t)) msg = "null d_edge_a, d_edge_b or d_t";
    else if (max_depth > LF_MKD_VIEW_GRAPH_MAX_ROUNDS) msg = "max_depth must be 0 .. 4096";
    else if (misaligned(3, d_edge_a, d_edge_b, d_t, d_rotations, d_image_stats, d_poses))
        msg = "the edge, translation, rotation, statistics and pose arrays must be 4-byte aligned";
    else if (above(kRowMax, n_images, n_edges)) msg = "n_images or n_edges above 2^31 - 1";
    else if (!h) msg = "null handle";
    if (msg) return refuse(h, "tree_poses_device", msg);
    if (n_images == 0) return LF_MKD_OK;
    LF_ENTER(h);
    launch_tree_poses(d_edge_a, d_edge_b, d_t, n_edges, d_rotations, d_image_stats, n_images, max_depth, d_poses, stream_of(h, stream));
    return launched(h);
}

// The host form: the arrays staged through the handle's d_ver_io with the poses, and the device call does the rest.
int lf_mkd_tree_poses(lf_mkd *h, const uint32_t *edge_a, const uint32_t *edge_b, const float *t, uint32_t n_edges,
                      const float *rotations, const uint32_t *image_stats, uint32_t n_images, uint32_t max_depth, float *poses) {
    const char *msg = nullptr;
    if (n_images && (!rotations || !image_stats || !poses)) msg = "null rotations, image_stats or poses";
    else if (n_images && n_edges && (!edge_a || !edge_b || !t)) msg = "null edge_a, edge_b or t";
    else if (max_depth > LF_MKD_VIEW_GRAPH_MAX_ROUNDS) msg = "max_depth must be 0 .. 4096";
    else if (above(kRowMax, n_images, n_edges)) msg = "n_images or n_edges above 2^31 - 1";
    else if (!h) msg = "null handle";
    if (msg) return refuse(h, "tree_poses", msg);
    if (n_images == 0) return LF_MKD_OK;
    LF_ENTER(h);
    Stager io(h, h->d_ver_io);
    const auto d_ea = io.part<uint32_t>(n_edges), d_eb = io.part<uint32_t>(n_edges);
    const auto d_t = io.part<float>(uint64_t(n_edges) * 3);
    const auto d_rot = io.part<float>(uint64_t(n_images) * 9);
    const auto d_is = io.part<uint32_t>(uint64_t(n_images) * 4);
    const auto d_poses = io.part<float>(uint64_t(n_images) * 12);
    if (int rc = io.reserve()) return rc;
    LF_HIP(h, io.up(d_ea, edge_a, n_edges));
    LF_HIP(h, io.up(d_eb, edge_b, n_edges));
    LF_HIP(h, io.up(d_t, t, uint64_t(n_edges) * 3));
    LF_HIP(h, io.up(d_rot, rotations, uint64_t(n_images) * 9));
    LF_HIP(h, io.up(d_is, image_stats, uint64_t(n_images) * 4));
    if (int rc = lf_mkd_tree_poses_device(h, d_ea, d_eb, d_t, n_edges, d_rot, d_is, n_images, max_depth, d_poses, h->stream)) return rc;
    LF_HIP(h, io.down(poses, d_poses, uint64_t(n_images) * 12));
    LF_HIP(h, hipStreamSynchronize(h->stream));
    return LF_MKD_OK;
}

// Global positions (csrc/mkd_positions.hip).  The sine of the robust angle is formed here, once, in double: no transcendental
// runs on the device (tests/cpp/positions_twin.cpp forms it with the same expression).
int lf_mkd_global_positions_plan(uint32_t n_images, uint64_t track_capacity, uint32_t sweeps, uint32_t *launches,
                                 uint64_t *scratch_bytes) {
    const char *msg = positions_sweeps_rule(sweeps);
    if (!msg && above(kRowMax, n_images, track_capacity)) msg = "n_images or track_capacity above 2^31 - 1";
    if (msg) return refuse(nullptr, "global_positions_plan", msg);
    const GlobalPositionsPlan p = global_positions_plan(n_images, track_capacity, sweeps);
    if (launches) *launches = p.launches;
    if (scratch_bytes) *scratch_bytes = p.scratch_bytes;
    return LF_MKD_OK;
}

int lf_mkd_global_positions_device(lf_mkd *h, const lf_mkd_keypoint *d_kps, const uint64_t *d_image_offsets, uint32_t n_images,
                                   uint64_t n_rows_total, const uint64_t *d_track_offsets, uint64_t track_capacity,
                                   const int32_t *d_obs_row, const uint32_t *d_obs_image, uint64_t obs_capacity,
                                   const uint32_t *d_table_counts, const int32_t *d_row_track, const float *d_intrinsics,
                                   const float *d_poses, uint32_t sweeps, uint32_t warm, float robust_deg, uint32_t min_obs,
                                   uint32_t flags, float *d_poses_out, float *d_points_out, uint32_t *d_obs_state,
                                   uint32_t *d_image_stats, double *d_trace, uint32_t *d_counts, void *stream) {
    const char *msg = nullptr;
    if (n_images && (!d_image_offsets || !d_table_counts || !d_intrinsics || !d_poses || !d_poses_out || !d_image_stats || !d_counts))
        msg = "null d_image_offsets, d_table_counts, d_intrinsics, d_poses, d_poses_out, d_image_stats or d_counts";
    else if (n_images && track_capacity && !d_track_offsets) msg = "null d_track_offsets";
    else if (n_images && track_capacity && obs_capacity && (!d_obs_row || !d_obs_image)) msg = "null d_obs_row or d_obs_image";
    else if (n_images && n_rows_total && (!d_kps || !d_row_track)) msg = "null d_kps or d_row_track";
    else if ((msg = positions_scalars(sweeps, robust_deg, min_obs, flags))) {}
    else if (misaligned(7, d_image_offsets) || misaligned(7, d_track_offsets) || misaligned(7, d_trace))
        msg = "d_image_offsets, d_track_offsets and d_trace must be 8-byte aligned";
    else if (misaligned(3, d_kps, d_obs_row, d_obs_image, d_table_counts, d_row_track, d_intrinsics, d_poses, d_poses_out, d_points_out,
                        d_obs_state, d_image_stats, d_counts))
        msg = "the keypoint, observation, count, track, intrinsics, pose, point, state, statistics and count arrays must be 4-byte aligned";
    else if (above(kRowMax, n_images, n_rows_total, track_capacity, obs_capacity)) msg = "a total or a capacity above 2^31 - 1";
    else if (!h) msg = "null handle";
    if (msg) return refuse(h, "global_positions_device", msg);
    if (n_images == 0) return LF_MKD_OK;
    LF_ENTER(h);
    const GlobalPositionsPlan plan = global_positions_plan(n_images, track_capacity, sweeps);
    unsigned char *work;
    if (int rc = scratch(h, h->d_positions, plan.scratch_bytes, &work)) return rc;
    const double s0 = std::sin(double(robust_deg) * (3.14159265358979323846 / 180.0));
    const SceneTables tables = {reinterpret_cast<const float *>(d_kps), n_rows_total, d_image_offsets, n_images, d_track_offsets,
                                track_capacity, d_obs_row, d_obs_image, obs_capacity, d_table_counts, d_row_track, d_intrinsics};
    const unsigned issued = launch_global_positions(plan, work, tables, d_poses, sweeps, warm, s0, min_obs, d_poses_out, d_points_out,
                                                    d_obs_state, d_image_stats, d_trace, d_counts, stream_of(h, stream));
    if (issued != plan.launches)
        return fail(h, LF_MKD_ERR_HIP, "global_positions_device: issued " + std::to_string(issued) + " launches, the plan says " +
                                           std::to_string(plan.launches));
    return launched(h);
}

// The host form: the arrays staged through the handle's d_ver_io with the outputs, counts = {n_tracks, n_obs}, in place on the
// staged poses.  The staged obs_state starts as zeros, so its entries outside every track's range come back 0.
int lf_mkd_global_positions(lf_mkd *h, const lf_mkd_keypoint *kps, const uint64_t *image_offsets, uint32_t n_images,
                            uint64_t n_rows_total, const uint64_t *track_offsets, uint64_t n_tracks, const int32_t *obs_row,
                            const uint32_t *obs_image, uint64_t n_obs, const int32_t *row_track, const float *intrinsics,
                            const float *poses, uint32_t sweeps, uint32_t warm, float robust_deg, uint32_t min_obs, uint32_t flags,
                            float *poses_out, float *points_out, uint32_t *obs_state, uint32_t *image_stats, double *trace,
                            uint32_t *counts) {
    const char *msg = nullptr;
    if (n_images && (!image_offsets || !intrinsics || !poses || !poses_out || !image_stats || !counts))
        msg = "null image_offsets, intrinsics, poses, poses_out, image_stats or counts";
    else if (n_images && n_tracks && !track_offsets) msg = "null track_offsets";
    else if (n_images && n_tracks && n_obs && (!obs_row || !obs_image)) msg = "null obs_row or obs_image";
    else if (n_images && n_rows_total && (!kps || !row_track)) msg = "null kps or row_track";
    else if ((msg = positions_scalars(sweeps, robust_deg, min_obs, flags))) {}
    else if (above(kRowMax, n_images, n_rows_total, n_tracks, n_obs)) msg = "a total above 2^31 - 1";
    else if (!h) msg = "null handle";
    if (msg) return refuse(h, "global_positions", msg);
    if (n_images == 0) return LF_MKD_OK;
    LF_ENTER(h);
    const uint64_t n_used = n_tracks ? n_obs : 0;
    Stager io(h, h->d_ver_io);
    const auto d_trace = io.part<double>(trace ? uint64_t(sweeps) * 4 : 0);
    const auto d_ioff = io.part<uint64_t>(uint64_t(n_images) + 1), d_toff = io.part<uint64_t>(n_tracks + 1);
    const auto d_tc = io.part<uint32_t>(2), d_counts = io.part<uint32_t>(8);
    const auto d_kps = io.part<lf_mkd_keypoint>(n_rows_total);
    const auto d_rt = io.part<int32_t>(n_rows_total);
    const auto d_row = io.part<int32_t>(n_used);
    const auto d_image = io.part<uint32_t>(n_used);
    const auto d_K = io.part<float>(uint64_t(n_images) * 4), d_poses = io.part<float>(uint64_t(n_images) * 12);
    const auto d_points = io.part<float>(points_out ? n_tracks * 4 : 0);
    const auto d_state = io.part<uint32_t>(obs_state ? n_used : 0);
    const auto d_is = io.part<uint32_t>(uint64_t(n_images) * 4);
    if (int rc = io.reserve()) return rc;
    const uint32_t tc[2] = {uint32_t(n_tracks), uint32_t(n_used)};
    LF_HIP(h, io.up(d_ioff, image_offsets, uint64_t(n_images) + 1));
    LF_HIP(h, io.up(d_toff, track_offsets, n_tracks ? n_tracks + 1 : 0));
    LF_HIP(h, io.up(d_tc, tc, 2));
    LF_HIP(h, io.up(d_kps, kps, n_rows_total));
    LF_HIP(h, io.up(d_rt, row_track, n_rows_total));
    LF_HIP(h, io.up(d_row, obs_row, n_used));
    LF_HIP(h, io.up(d_image, obs_image, n_used));
    LF_HIP(h, io.up(d_K, intrinsics, uint64_t(n_images) * 4));
    LF_HIP(h, io.up(d_poses, poses, uint64_t(n_images) * 12));
    if (obs_state && n_used) LF_HIP(h, hipMemsetAsync(d_state.get(), 0, n_used * 4, h->stream));
    if (int rc = lf_mkd_global_positions_device(h, d_kps, d_ioff, n_images, n_rows_total, d_toff, n_tracks, d_row, d_image, n_used, d_tc,
                                                d_rt, d_K, d_poses, sweeps, warm, robust_deg, min_obs, flags, d_poses,
                                                points_out ? d_points.get() : nullptr, obs_state ? d_state.get() : nullptr, d_is,
                                                trace ? d_trace.get() : nullptr, d_counts, h->stream))
        return rc;
    LF_HIP(h, io.down(poses_out, d_poses, uint64_t(n_images) * 12));
    LF_HIP(h, io.down(points_out, d_points, points_out ? n_tracks * 4 : 0));
    LF_HIP(h, io.down(obs_state, d_state, obs_state ? n_used : 0));
    LF_HIP(h, io.down(image_stats, d_is, uint64_t(n_images) * 4));
    LF_HIP(h, io.down(trace, d_trace, trace ? uint64_t(sweeps) * 4 : 0));
    LF_HIP(h, io.down(counts, d_counts, 8));
    LF_HIP(h, hipStreamSynchronize(h->stream));
    return LF_MKD_OK;
}

}  // extern "C"
