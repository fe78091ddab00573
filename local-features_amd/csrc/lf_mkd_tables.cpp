// C ABI, the tables built from matches: tracks, track tables, track descriptors, link tables, candidate edges, covisibility.
#include <cmath>

#include "lf_mkd_args.h"
#include "mkd_consts.hpp"
#include "mkd_scene.h"

extern "C" {

// Feature tracks over an edge list's matches (csrc/mkd_tracks.hip).  The grids are sized here, from the arguments alone.
int lf_mkd_build_tracks_device(lf_mkd *h, const uint64_t *d_image_offsets, uint32_t n_images, uint64_t n_rows_total,
                               const uint32_t *d_edge_a, const uint32_t *d_edge_b, const uint64_t *d_edge_offsets_a,
                               uint64_t ea_capacity, uint32_t n_edges, const int32_t *d_match, uint32_t flags,
                               int32_t *d_track, uint32_t *d_track_len, uint32_t *d_track_dup, void *stream) {
    const char *msg = nullptr;
    if (!d_image_offsets || !d_track) msg = "null pointer";
    else if (n_edges && (!d_edge_a || !d_edge_b)) msg = "null edge array";
    else if (n_edges && !d_edge_offsets_a) msg = "null layout array";
    else if (n_edges && !d_match) msg = "null match array";
    else if (misaligned(7, d_image_offsets, d_edge_offsets_a)) msg = "the offset arrays must be 8-byte aligned";
    else if (misaligned(3, d_edge_a, d_edge_b, d_match, d_track, d_track_len, d_track_dup))
        msg = "the edge, match, track and statistics arrays must be 4-byte aligned";
    else if (flags & ~LF_MKD_TRACKS_ACCUMULATE) msg = "unknown flag bits";
    else if (above(kRowMax, n_rows_total, ea_capacity)) msg = "a total or a capacity above 2^31 - 1 rows";
    else if (above(kRowMax, ea_capacity / build_tracks_link_entries() + n_edges))
        msg = "too many entries and edges for one call (the link grid needs floor(ea_capacity / 256) + n_edges workgroups, at "
              "most 2^31 - 1)";
    else if (d_track_dup && above(kRowMax, n_rows_total / build_tracks_dup_tile() + n_images))
        msg = "too many rows and images for one call (d_track_dup's grid needs floor(n_rows_total / LF_MKD_TRACKS_DUP_TILE) + "
              "n_images workgroups, at most 2^31 - 1)";
    else if (!h) msg = "null handle";
    if (msg) return refuse(h, "build_tracks_device", msg);
    if (n_rows_total == 0) return LF_MKD_OK;
    LF_ENTER(h);
    launch_build_tracks(d_image_offsets, n_images, n_rows_total, d_edge_a, d_edge_b, d_edge_offsets_a, ea_capacity, n_edges,
                        d_match, (flags & LF_MKD_TRACKS_ACCUMULATE) != 0, d_track, d_track_len, d_track_dup, stream_of(h, stream));
    return launched(h);
}

// Track tables (csrc/mkd_track_table.hip).
int lf_mkd_track_table_plan(uint64_t n_rows_total, uint32_t min_len, uint32_t *key_bits, uint32_t *passes, uint32_t *block_rows,
                            uint64_t *scratch_bytes) {
    if (min_len == 0) return refuse(nullptr, "track_table_plan", "min_len must be at least 1");
    if (above(kRowMax, n_rows_total)) return refuse(nullptr, "track_table_plan", "more than 2^31 - 1 rows in the pool");
    const TrackTablePlan p = track_table_plan(n_rows_total, min_len);
    if (key_bits) *key_bits = p.key_bits;
    if (passes) *passes = p.passes;
    if (block_rows) *block_rows = p.block_rows;
    if (scratch_bytes) *scratch_bytes = p.scratch_bytes;
    return LF_MKD_OK;
}

int lf_mkd_track_table_device(lf_mkd *h, const uint64_t *d_image_offsets, uint32_t n_images, uint64_t n_rows_total,
                              const int32_t *d_track, const uint32_t *d_track_len, const uint32_t *d_track_dup, uint32_t min_len,
                              uint32_t flags, uint64_t track_capacity, uint64_t obs_capacity, uint64_t *d_track_offsets,
                              int32_t *d_obs_row, uint32_t *d_obs_image, int32_t *d_row_track, uint32_t *d_counts, void *stream) {
    const bool consistent = flags & LF_MKD_TRACK_TABLE_CONSISTENT;
    const char *msg = nullptr;
    if (!d_track_offsets || !d_counts) msg = "null pointer";
    else if (n_rows_total && (!d_track || !d_track_len)) msg = "null track or length array";
    else if (obs_capacity && !d_obs_row) msg = "null d_obs_row";
    else if (d_obs_image && !d_image_offsets) msg = "d_obs_image needs d_image_offsets";
    else if (min_len == 0) msg = "min_len must be at least 1";
    else if (flags & ~LF_MKD_TRACK_TABLE_CONSISTENT) msg = "unknown flag bits";
    else if (consistent && n_rows_total && !d_track_dup) msg = "LF_MKD_TRACK_TABLE_CONSISTENT needs d_track_dup";
    else if (misaligned(7, d_image_offsets, d_track_offsets)) msg = "the offset arrays must be 8-byte aligned";
    else if (misaligned(3, d_track, d_track_len, d_track_dup, d_obs_row, d_obs_image, d_row_track, d_counts))
        msg = "the track, statistics, observation and count arrays must be 4-byte aligned";
    else if (above(kRowMax, n_rows_total, track_capacity, obs_capacity)) msg = "a total or a capacity above 2^31 - 1";
    else if (!h) msg = "null handle";
    if (msg) return refuse(h, "track_table_device", msg);
    LF_ENTER(h);
    const TrackTablePlan plan = track_table_plan(n_rows_total, min_len);
    unsigned char *work;
    if (int rc = scratch(h, h->d_track_table, plan.scratch_bytes, &work)) return rc;
    launch_track_table(plan, work, d_image_offsets, n_images, n_rows_total, d_track, d_track_len, consistent ? d_track_dup : nullptr,
                       min_len, track_capacity, obs_capacity, d_track_offsets, d_obs_row, d_obs_image, d_row_track, d_counts,
                       stream_of(h, stream));
    return launched(h);
}

int lf_mkd_gather_track_rows_device(lf_mkd *h, const void *d_src, uint32_t row_bytes, uint64_t n_rows_total,
                                    const int32_t *d_obs_row, const uint32_t *d_counts, uint64_t obs_capacity, void *d_dst,
                                    void *stream) {
    const char *msg = nullptr;
    if (!d_counts || (n_rows_total && !d_src) || (obs_capacity && (!d_obs_row || !d_dst))) msg = "null pointer";
    else if (row_bytes < 4 || row_bytes > 512 || (row_bytes & 3)) msg = "row_bytes must be a multiple of 4 in [4, 512]";
    else if (misaligned(3, d_src, d_dst, d_obs_row, d_counts)) msg = "every array must be 4-byte aligned";
    else if (above(kRowMax, n_rows_total, obs_capacity)) msg = "a total or a capacity above 2^31 - 1";
    else if (!h) msg = "null handle";
    if (msg) return refuse(h, "gather_track_rows_device", msg);
    if (obs_capacity == 0) return LF_MKD_OK;
    LF_ENTER(h);
    launch_gather_track_rows(d_src, row_bytes, n_rows_total, d_obs_row, d_counts, obs_capacity, d_dst, stream_of(h, stream));
    return launched(h);
}

// Track descriptors (csrc/mkd_track_desc.hip).  The parallax cosine is formed here, once, in double, with resection's
// expression (tests/cpp/track_desc_twin.cpp forms it with the same one).
int lf_mkd_track_descriptors_device(lf_mkd *h, const uint8_t *d_q, uint64_t n_rows_total, const uint64_t *d_track_offsets,
                                    uint64_t track_capacity, const int32_t *d_obs_row, uint64_t obs_capacity,
                                    const uint32_t *d_table_counts, const uint32_t *d_obs_state, uint32_t min_state,
                                    const float *d_points, float min_parallax_deg, float scale, uint8_t *d_desc,
                                    int32_t *d_desc_stats, void *stream) {
    const char *msg = nullptr;
    if (track_capacity && (!d_track_offsets || !d_table_counts || !d_desc)) msg = "null d_track_offsets, d_table_counts or d_desc";
    else if (track_capacity && obs_capacity && !d_obs_row) msg = "null d_obs_row";
    else if (track_capacity && obs_capacity && n_rows_total && !d_q) msg = "null d_q";
    else if ((msg = track_desc_scalars(min_state, min_parallax_deg, scale))) {}
    else if (misaligned(15, d_q, d_desc)) msg = "d_q and d_desc must be 16-byte aligned";
    else if (misaligned(7, d_track_offsets)) msg = "d_track_offsets must be 8-byte aligned";
    else if (misaligned(3, d_obs_row, d_table_counts, d_obs_state, d_points, d_desc_stats))
        msg = "the observation, count, state, point and statistics arrays must be 4-byte aligned";
    else if (above(kRowMax, n_rows_total, track_capacity, obs_capacity)) msg = "a total or a capacity above 2^31 - 1";
    else if (!h) msg = "null handle";
    if (msg) return refuse(h, "track_descriptors_device", msg);
    if (track_capacity == 0) return LF_MKD_OK;
    LF_ENTER(h);
    const double cmin = std::cos(double(min_parallax_deg) * (3.14159265358979323846 / 180.0));
    const SceneTables tables = {nullptr, n_rows_total, nullptr, 0, d_track_offsets, track_capacity, d_obs_row, nullptr,
                                obs_capacity, d_table_counts, nullptr, nullptr};
    launch_track_descriptors(tables, d_q, d_obs_state, min_state, d_points, cmin, scale, d_desc, d_desc_stats, stream_of(h, stream));
    return launched(h);
}

// The host form: the arrays staged through the handle's d_ver_io with the outputs, counts = {n_tracks, n_obs}, and the device
// call does the rest.
int lf_mkd_track_descriptors(lf_mkd *h, const uint8_t *q, uint64_t n_rows_total, const uint64_t *track_offsets, uint64_t n_tracks,
                             const int32_t *obs_row, uint64_t n_obs, const uint32_t *obs_state, uint32_t min_state,
                             const float *points, float min_parallax_deg, float scale, uint8_t *desc, int32_t *desc_stats) {
    const char *msg = nullptr;
    if (n_tracks && (!track_offsets || !desc)) msg = "null track_offsets or desc";
    else if (n_tracks && n_obs && !obs_row) msg = "null obs_row";
    else if (n_tracks && n_obs && n_rows_total && !q) msg = "null q";
    else if ((msg = track_desc_scalars(min_state, min_parallax_deg, scale))) {}
    else if (above(kRowMax, n_rows_total, n_tracks, n_obs)) msg = "a total above 2^31 - 1";
    else if (!h) msg = "null handle";
    if (msg) return refuse(h, "track_descriptors", msg);
    if (n_tracks == 0) return LF_MKD_OK;
    LF_ENTER(h);
    // counts [2], the arrays in the device call's order, then the outputs
    const uint64_t rows_up = n_obs ? n_rows_total : 0;
    Stager io(h, h->d_ver_io);
    const auto d_counts = io.part<uint32_t>(2);
    const auto d_offs = io.part<uint64_t>(n_tracks + 1);
    const auto d_q = io.part<uint8_t>(rows_up * 128);
    const auto d_row = io.part<int32_t>(n_obs);
    const auto d_state = io.part<uint32_t>(obs_state ? n_obs : 0);
    const auto d_points = io.part<float>(points ? n_tracks * 4 : 0);
    const auto d_desc = io.part<uint8_t>(n_tracks * 128);
    const auto d_stats = io.part<int32_t>(desc_stats ? n_tracks * 2 : 0);
    if (int rc = io.reserve()) return rc;
    // (counts saturate: the totals are below 2^31)
    const uint32_t counts[2] = {uint32_t(n_tracks), uint32_t(n_obs)};
    LF_HIP(h, io.up(d_counts, counts, 2));
    LF_HIP(h, io.up(d_offs, track_offsets, n_tracks + 1));
    LF_HIP(h, io.up(d_q, q, rows_up * 128));
    LF_HIP(h, io.up(d_row, obs_row, n_obs));
    LF_HIP(h, io.up(d_state, obs_state, obs_state ? n_obs : 0));
    LF_HIP(h, io.up(d_points, points, points ? n_tracks * 4 : 0));
    if (int rc = lf_mkd_track_descriptors_device(h, d_q, n_rows_total, d_offs, n_tracks, d_row, n_obs, d_counts,
                                                 obs_state ? d_state.get() : nullptr, min_state, points ? d_points.get() : nullptr,
                                                 min_parallax_deg, scale, d_desc, desc_stats ? d_stats.get() : nullptr, h->stream))
        return rc;
    LF_HIP(h, io.down(desc, d_desc, n_tracks * 128));
    LF_HIP(h, io.down(desc_stats, d_stats, desc_stats ? n_tracks * 2 : 0));
    LF_HIP(h, hipStreamSynchronize(h->stream));
    return LF_MKD_OK;
}

// Link tables (csrc/mkd_link_table.hip); the grid is tracks_link's.
static const char *link_table_sizes(uint64_t ea_capacity, uint32_t n_edges) {
    if (above(kRowMax, ea_capacity)) return "a total or a capacity above 2^31 - 1";
    if (above(kRowMax, ea_capacity / link_table_plan(0, 0).slot_entries + n_edges))
        return "too many entries and edges for one call (the grid needs floor(ea_capacity / slot_entries) + n_edges workgroups, at "
               "most 2^31 - 1)";
    return nullptr;
}

int lf_mkd_link_table_plan(uint64_t ea_capacity, uint32_t n_edges, uint32_t *slot_entries, uint64_t *slots,
                           uint32_t *scan_fanout, uint32_t *scan_levels, uint64_t *scratch_bytes) {
    if (const char *msg = link_table_sizes(ea_capacity, n_edges)) return refuse(nullptr, "link_table_plan", msg);
    const LinkTablePlan p = link_table_plan(ea_capacity, n_edges);
    if (slot_entries) *slot_entries = p.slot_entries;
    if (slots) *slots = p.slots;
    if (scan_fanout) *scan_fanout = p.scan_fanout;
    if (scan_levels) *scan_levels = p.scan_levels;
    if (scratch_bytes) *scratch_bytes = p.scratch_bytes;
    return LF_MKD_OK;
}

int lf_mkd_link_table_device(lf_mkd *h, const uint64_t *d_image_offsets, uint32_t n_images, uint64_t n_rows_total,
                             const uint32_t *d_edge_a, const uint32_t *d_edge_b, const uint64_t *d_edge_offsets_a,
                             uint64_t ea_capacity, uint32_t n_edges, const int32_t *d_match, uint32_t min_links,
                             uint32_t flags, uint64_t link_capacity, uint64_t *d_link_offsets, int32_t *d_link_a,
                             int32_t *d_link_b, uint32_t *d_link_edge, uint32_t *d_edge_links, int32_t *d_match_kept,
                             uint32_t *d_counts, void *stream) {
    const char *msg = nullptr;
    if (!d_image_offsets || !d_link_offsets || !d_counts) msg = "null pointer";
    else if (n_edges && (!d_edge_a || !d_edge_b)) msg = "null edge array";
    else if (n_edges && !d_edge_offsets_a) msg = "null layout array";
    else if (n_edges && !d_match) msg = "null match array";
    else if (link_capacity && (!d_link_a || !d_link_b)) msg = "null d_link_a or d_link_b";
    else if (flags & ~LF_MKD_LINK_TABLE_LOCAL) msg = "unknown flag bits";
    else if (misaligned(7, d_image_offsets, d_edge_offsets_a, d_link_offsets)) msg = "the offset arrays must be 8-byte aligned";
    else if (misaligned(3, d_edge_a, d_edge_b, d_match, d_link_a, d_link_b, d_link_edge, d_edge_links, d_match_kept, d_counts))
        msg = "the edge, match, link and count arrays must be 4-byte aligned";
    else if (above(kRowMax, n_rows_total, link_capacity)) msg = "a total or a capacity above 2^31 - 1";
    else if (!(msg = link_table_sizes(ea_capacity, n_edges)) && !h) msg = "null handle";
    if (msg) return refuse(h, "link_table_device", msg);
    LF_ENTER(h);
    const LinkTablePlan plan = link_table_plan(ea_capacity, n_edges);
    unsigned char *work;
    if (int rc = scratch(h, h->d_link_table, plan.scratch_bytes, &work)) return rc;
    launch_link_table(plan, work, d_image_offsets, n_images, n_rows_total, d_edge_a, d_edge_b, d_edge_offsets_a, ea_capacity, n_edges,
                      d_match, min_links, (flags & LF_MKD_LINK_TABLE_LOCAL) != 0, link_capacity, d_link_offsets, d_link_a, d_link_b,
                      d_link_edge, d_edge_links, d_match_kept, d_counts, stream_of(h, stream));
    return launched(h);
}

// Candidate edges (csrc/mkd_select_edges.hip).
static const char *select_edges_sizes(uint32_t n_a, uint32_t n_b, uint32_t k, uint64_t edge_capacity, uint32_t flags) {
    if (k == 0 || k > LF_MKD_SELECT_MAX_K) return "k must be in [1, 32]";
    if (flags & ~(LF_MKD_SELECT_SKIP_SELF | LF_MKD_SELECT_UNIQUE)) return "unknown flag bits";
    if ((flags & LF_MKD_SELECT_UNIQUE) && n_a != n_b) return "LF_MKD_SELECT_UNIQUE needs one pool (n_a == n_b)";
    if (n_a && n_b == 0) return "n_b == 0 with n_a > 0";
    if (above(kRowMax, uint64_t(n_a) * n_b)) return "a table of more than 2^31 - 1 entries (n_a * n_b)";
    if (above(kRowMax, uint64_t(n_a) * k, edge_capacity)) return "n_a * k or edge_capacity above 2^31 - 1";
    return nullptr;
}

int lf_mkd_select_edges_plan(uint32_t n_a, uint32_t n_b, uint32_t k, uint64_t edge_capacity, uint32_t flags,
                             uint32_t *compiled_k, uint32_t *rows_per_workgroup, uint64_t *workgroups, uint32_t *launches,
                             uint64_t *scratch_bytes) {
    if (const char *msg = select_edges_sizes(n_a, n_b, k, edge_capacity, flags)) return refuse(nullptr, "select_edges_plan", msg);
    const SelectEdgesPlan p = select_edges_plan(n_a, n_b, k, edge_capacity);
    if (compiled_k) *compiled_k = p.compiled_k;
    if (rows_per_workgroup) *rows_per_workgroup = p.rows_per_workgroup;
    if (workgroups) *workgroups = p.workgroups;
    if (launches) *launches = p.launches;
    if (scratch_bytes) *scratch_bytes = p.scratch_bytes;
    return LF_MKD_OK;
}

int lf_mkd_select_edges_device(lf_mkd *h, const uint32_t *d_votes, uint32_t n_a, uint32_t n_b, uint32_t k, uint32_t min_votes,
                               uint32_t flags, uint64_t edge_capacity, int32_t *d_rank, uint32_t *d_rank_votes,
                               uint32_t *d_edge_a, uint32_t *d_edge_b, uint32_t *d_edge_votes, uint32_t *d_counts, void *stream) {
    const char *msg = nullptr;
    if (n_a && !d_votes) msg = "null d_votes";
    else if (!d_counts) msg = "null d_counts";
    else if (edge_capacity && (!d_edge_a || !d_edge_b)) msg = "null d_edge_a or d_edge_b";
    else if (misaligned(3, d_votes, d_rank, d_rank_votes, d_edge_a, d_edge_b, d_edge_votes, d_counts))
        msg = "every array must be 4-byte aligned";
    else if (!(msg = select_edges_sizes(n_a, n_b, k, edge_capacity, flags)) && !h) msg = "null handle";
    if (msg) return refuse(h, "select_edges_device", msg);
    LF_ENTER(h);
    const SelectEdgesPlan plan = select_edges_plan(n_a, n_b, k, edge_capacity);
    unsigned char *work;
    if (int rc = scratch(h, h->d_select_edges, plan.scratch_bytes, &work)) return rc;
    launch_select_edges(plan, work, d_votes, n_a, n_b, k, min_votes, (flags & LF_MKD_SELECT_SKIP_SELF) != 0,
                        (flags & LF_MKD_SELECT_UNIQUE) != 0, edge_capacity, d_rank, d_rank_votes, d_edge_a, d_edge_b, d_edge_votes,
                        d_counts, stream_of(h, stream));
    return launched(h);
}

// Covisibility tables (csrc/mkd_covisibility.hip).
static const char *covisibility_sizes(uint32_t n_images, uint64_t track_capacity, uint64_t obs_capacity, uint32_t flags) {
    if (flags & ~LF_MKD_COVIS_ACCUMULATE) return "unknown flag bits";
    if (above(kRowMax, uint64_t(n_images) * n_images)) return "a table of more than 2^31 - 1 entries (n_images^2)";
    if (above(kRowMax, track_capacity, obs_capacity)) return "track_capacity or obs_capacity above 2^31 - 1";
    return nullptr;
}

int lf_mkd_covisibility_plan(uint32_t n_images, uint64_t track_capacity, uint64_t obs_capacity, uint64_t n_edges, uint32_t flags,
                             uint32_t *form, uint64_t *workgroups, uint32_t *launches, uint64_t *scratch_bytes) {
    if (const char *msg = covisibility_sizes(n_images, track_capacity, obs_capacity, flags))
        return refuse(nullptr, "covisibility_plan", msg);
    const CovisibilityPlan p = covisibility_plan(n_images, track_capacity, obs_capacity, n_edges);
    if (form) *form = p.group | (p.lds ? LF_MKD_COVIS_FORM_LDS : 0u);
    if (workgroups) *workgroups = p.short_blocks;
    if (launches) *launches = p.launches;
    if (scratch_bytes) *scratch_bytes = p.scratch_bytes;
    return LF_MKD_OK;
}

int lf_mkd_covisibility_device(lf_mkd *h, const uint64_t *d_track_offsets, uint64_t track_capacity, const uint32_t *d_obs_image,
                               uint64_t obs_capacity, const uint32_t *d_table_counts, uint32_t n_images, const uint32_t *d_edge_a,
                               const uint32_t *d_edge_b, uint64_t n_edges, uint32_t flags, uint32_t *d_covis, void *stream) {
    const char *msg = nullptr;
    if (n_images && !d_covis) msg = "null d_covis";
    else if (!d_table_counts) msg = "null d_table_counts";
    else if (!d_track_offsets) msg = "null d_track_offsets";
    else if (obs_capacity && !d_obs_image) msg = "null d_obs_image";
    else if (!d_edge_a != !d_edge_b) msg = "only one of d_edge_a and d_edge_b";
    else if (n_edges && !d_edge_a) msg = "n_edges > 0 without d_edge_a and d_edge_b";
    else if (misaligned(7, d_track_offsets)) msg = "d_track_offsets must be 8-byte aligned";
    else if (misaligned(3, d_obs_image, d_table_counts, d_edge_a, d_edge_b, d_covis))
        msg = "the observation, count, edge and table arrays must be 4-byte aligned";
    else if (!(msg = covisibility_sizes(n_images, track_capacity, obs_capacity, flags)) && !h) msg = "null handle";
    if (msg) return refuse(h, "covisibility_device", msg);
    if (n_images == 0) return LF_MKD_OK;
    LF_ENTER(h);
    const CovisibilityPlan plan = covisibility_plan(n_images, track_capacity, obs_capacity, n_edges);
    unsigned char *work;
    if (int rc = scratch(h, h->d_covisibility, plan.scratch_bytes, &work)) return rc;
    launch_covisibility(plan, work, d_track_offsets, track_capacity, d_obs_image, obs_capacity, d_table_counts, n_images, d_edge_a,
                        d_edge_b, n_edges, (flags & LF_MKD_COVIS_ACCUMULATE) != 0, d_covis, stream_of(h, stream));
    return launched(h);
}

}  // extern "C"
