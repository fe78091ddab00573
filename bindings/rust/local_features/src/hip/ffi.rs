//! Raw declarations of `include/lf_mkd.h` (liblf_mkd.so, the MI355X-native MKD path): one `extern "C"` item per entry
//! point of the header, `#[repr(C)]` twins of its structs.  `tests/test_rust_binding.py` checks every item here against
//! the header (name, arity, pointer/scalar class of each argument), and the struct layouts against `offsetof`.
//!
//! New file in the reference tree: `local_features/src/hip/ffi.rs`.
#![allow(non_camel_case_types, dead_code)]

use std::os::raw::{c_char, c_int, c_void};

pub const LF_MKD_OK: c_int = 0;
pub const LF_MKD_ERR_BAD_ARG: c_int = -1;
pub const LF_MKD_ERR_HIP: c_int = -2;
pub const LF_MKD_ERR_IO: c_int = -3;
pub const LF_MKD_ERR_NO_IMAGE: c_int = -4;
pub const LF_MKD_ERR_NO_DEVICE: c_int = -5;
pub const LF_MKD_ERR_COMM: c_int = -6;

pub const LF_MKD_ANGLE_SHADER: i32 = 0;
pub const LF_MKD_ANGLE_EXACT: i32 = 1;
pub const LF_MKD_ANGLE_EXACT_ZERO: i32 = 2;
pub const LF_MKD_POOL_DEFAULT: i32 = 0;
pub const LF_MKD_POOL_F16X3: i32 = 1;
pub const LF_MKD_POOL_F32: i32 = 2;
pub const LF_MKD_POOL_F16_FP6: i32 = 3;
pub const LF_MKD_FLAG_KERNEL_TIMING: u32 = 1;
pub const LF_MKD_FLAG_UNFUSED_KEYPOINTS: u32 = 2;
pub const LF_MKD_FLAG_DETECT_STEPWISE: u32 = 4;
pub const LF_MKD_MAX_ANGLES_PER_EXTREMUM: usize = 18;
pub const LF_MKD_COMM_ID_BYTES: usize = 128;
pub const LF_MKD_GATHER_DIRECT: i32 = 0;
pub const LF_MKD_GATHER_RING: i32 = 1;

/// `lf_mkd_params`: BuildTimeParams (lib.rs:54-75) + FeatureDetectParams (lib.rs:34-52) for this path; 0 = default.
#[repr(C)]
#[derive(Debug, Clone, Copy, Default)]
pub struct lf_mkd_params {
    pub max_image_width: u32,
    pub max_image_height: u32,
    pub max_features: u32,
    pub patch_scale_factor: f32,
    pub device: i32,
    pub angle_mode: i32,
    pub pool_mode: i32,
    pub flags: u32,
    pub max_frames: u32,
    pub n_scales: u32,
    pub max_blobs: u32,
    pub reserved: [u32; 1],
}

/// `lf_mkd_keypoint`: layout-identical to `crate::Keypoint` (lib.rs:17-24), angle in degrees.
#[repr(C)]
#[derive(Debug, Clone, Copy, Default, PartialEq)]
pub struct lf_mkd_keypoint {
    pub x: f32,
    pub y: f32,
    pub size: f32,
    pub angle: f32,
    pub response: f32,
}

/// `lf_mkd_extremum`: one refined blob {x, y, interpolated scale, contrast} (ExtremumLocations, common.glsl:45-81).
#[repr(C)]
#[derive(Debug, Clone, Copy, Default, PartialEq)]
pub struct lf_mkd_extremum {
    pub x: f32,
    pub y: f32,
    pub size: f32,
    pub response: f32,
}

/// Opaque handle; owns all device memory.
#[repr(C)]
pub struct lf_mkd {
    _private: [u8; 0],
}

/// Opaque RCCL communicator of one rank (`lf_mkd_comm_create`).
#[repr(C)]
pub struct lf_mkd_comm {
    _private: [u8; 0],
}

extern "C" {
    pub fn lf_mkd_create(params: *const lf_mkd_params, mean: *const f32, eigvals: *const f32, eigvecs: *const f32,
                         out: *mut *mut lf_mkd) -> c_int;
    pub fn lf_mkd_create_from_file(params: *const lf_mkd_params, safetensors_path: *const c_char,
                                   out: *mut *mut lf_mkd) -> c_int;
    pub fn lf_mkd_destroy(h: *mut lf_mkd);
    pub fn lf_mkd_last_error(h: *const lf_mkd) -> *const c_char;

    pub fn lf_mkd_describe_patches(h: *mut lf_mkd, patches: *const f32, n: u64, out: *mut f32) -> c_int;
    pub fn lf_mkd_describe_patches_device(h: *mut lf_mkd, d_patches: *const f32, n: u64, d_out: *mut f32,
                                          stream: *mut c_void) -> c_int;
    pub fn lf_mkd_raw_descriptors_device(h: *mut lf_mkd, d_patches: *const f32, n: u64, d_raw: *mut f32,
                                         stream: *mut c_void) -> c_int;

    pub fn lf_mkd_set_image(h: *mut lf_mkd, image: *const f32, width: u32, height: u32) -> c_int;
    pub fn lf_mkd_set_image_device(h: *mut lf_mkd, d_image: *const f32, width: u32, height: u32,
                                   stream: *mut c_void) -> c_int;
    pub fn lf_mkd_set_images_device(h: *mut lf_mkd, d_images: *const f32, n_frames: u32, width: u32, height: u32,
                                    stream: *mut c_void) -> c_int;
    pub fn lf_mkd_set_image_u8(h: *mut lf_mkd, image: *const u8, width: u32, height: u32) -> c_int;
    pub fn lf_mkd_set_images_u8_device(h: *mut lf_mkd, d_images: *const u8, n_frames: u32, width: u32, height: u32,
                                       stream: *mut c_void) -> c_int;

    pub fn lf_mkd_describe_keypoints(h: *mut lf_mkd, kps: *const lf_mkd_keypoint, n: u64, out: *mut f32) -> c_int;
    pub fn lf_mkd_describe_keypoints_device(h: *mut lf_mkd, d_kps: *const lf_mkd_keypoint, n: u64, d_out: *mut f32,
                                            stream: *mut c_void) -> c_int;
    pub fn lf_mkd_describe_keypoints_frames_device(h: *mut lf_mkd, d_kps: *const lf_mkd_keypoint,
                                                   d_frame_of_kp: *const u32, n: u64, d_out: *mut f32,
                                                   stream: *mut c_void) -> c_int;

    pub fn lf_mkd_orient_keypoints(h: *mut lf_mkd, extrema: *const lf_mkd_extremum, n: u64,
                                   out: *mut lf_mkd_keypoint, max_out: u64, n_out: *mut u64,
                                   n_dropped: *mut u64) -> c_int;
    pub fn lf_mkd_orient_keypoints_device(h: *mut lf_mkd, d_extrema: *const lf_mkd_extremum,
                                          d_frame_of_extremum: *const u32, n: u64, d_out: *mut lf_mkd_keypoint,
                                          d_frame_of_kp: *mut u32, max_out: u64, n_out: *mut u64,
                                          n_dropped: *mut u64, stream: *mut c_void) -> c_int;
    pub fn lf_mkd_orient_keypoints_blocked(h: *mut lf_mkd, extremum_data: *const f32, n_extrema: u64, block_len: u32,
                                           indices: *const u32, n_indices: u64, kp_extremum_index: *mut u32,
                                           kp_orientation: *mut f32, keypoints: *mut lf_mkd_keypoint, max_out: u64,
                                           n_out: *mut u64, n_dropped: *mut u64) -> c_int;

    pub fn lf_mkd_detect_extrema_device(h: *mut lf_mkd, d_out: *mut lf_mkd_extremum, d_frame_of: *mut u32,
                                        max_out: u64, n_out: *mut u64, n_dropped: *mut u64,
                                        stream: *mut c_void) -> c_int;
    pub fn lf_mkd_detect_extrema(h: *mut lf_mkd, out: *mut lf_mkd_extremum, max_out: u64, n_out: *mut u64,
                                 n_dropped: *mut u64) -> c_int;
    pub fn lf_mkd_filter_extrema_device(h: *mut lf_mkd, d_extrema: *const lf_mkd_extremum, n: u64, top_n: u32,
                                        min_size: f32, d_out: *mut lf_mkd_extremum, d_index: *mut u32,
                                        n_out: *mut u64, stream: *mut c_void) -> c_int;

    pub fn lf_mkd_detect(h: *mut lf_mkd, image: *const f32, width: u32, height: u32, top_n: u32, min_size: f32,
                         keypoints: *mut lf_mkd_keypoint, descriptors: *mut f32, max_out: u64, n_out: *mut u64,
                         dropped_blobs: *mut u64, dropped_features: *mut u64) -> c_int;
    pub fn lf_mkd_detect_u8(h: *mut lf_mkd, image: *const u8, width: u32, height: u32, top_n: u32, min_size: f32,
                            keypoints: *mut lf_mkd_keypoint, descriptors: *mut f32, max_out: u64, n_out: *mut u64,
                            dropped_blobs: *mut u64, dropped_features: *mut u64) -> c_int;
    pub fn lf_mkd_detect_times(h: *mut lf_mkd, upload_ms: *mut f64, pipeline_ms: *mut f64, readback_ms: *mut f64) -> c_int;
    pub fn lf_mkd_detect_frames_device(h: *mut lf_mkd, d_images: *const f32, n_frames: u32, width: u32, height: u32,
                                       top_n: u32, min_size: f32, d_keypoints: *mut lf_mkd_keypoint,
                                       d_frame_of_kp: *mut u32, d_descriptors: *mut f32, max_out: u64,
                                       n_out: *mut u64, dropped_blobs: *mut u64, dropped_features: *mut u64,
                                       stream: *mut c_void) -> c_int;

    pub fn lf_mkd_stream_create(h: *mut lf_mkd, width: u32, height: u32, top_n: u32, min_size: f32, max_out: u64,
                                d_image: *const f32, d_keypoints: *mut lf_mkd_keypoint, d_descriptors: *mut f32,
                                d_counts: *mut u64) -> c_int;
    pub fn lf_mkd_stream_frame(h: *mut lf_mkd, stream: *mut c_void) -> c_int;

    pub fn lf_mkd_match_device(h: *mut lf_mkd, d_a: *const f32, na: u64, d_b: *const f32, nb: u64,
                               d_exclude_lo: *const u32, d_exclude_hi: *const u32, ratio: f32, d_match: *mut i32,
                               d_best: *mut f32, d_second: *mut f32, stream: *mut c_void) -> c_int;
    pub fn lf_mkd_match_both_device(h: *mut lf_mkd, d_a: *const f32, na: u64, d_b: *const f32, nb: u64, ratio: f32,
                                    d_match_ab: *mut i32, d_match_ba: *mut i32, stream: *mut c_void) -> c_int;
    // n_pairs match problems in one launch, in the batched verifiers' layout (offsets on the device); flags: LF_MKD_MATCH_MUTUAL
    pub fn lf_mkd_match_pairs_device(h: *mut lf_mkd, d_a: *const f32, d_offsets_a: *const u64, na_total: u64,
                                     d_b: *const f32, d_offsets_b: *const u64, nb_total: u64, n_pairs: u32, ratio: f32,
                                     flags: u32, d_match_ab: *mut i32, d_match_ba: *mut i32, d_best: *mut f32,
                                     d_second: *mut f32, stream: *mut c_void) -> c_int;
    // the same batch under each pair's verified model (d_model [n_pairs][9], kind: GUIDE_HOMOGRAPHY / GUIDE_FUNDAMENTAL of
    // mod.rs): a row's candidates are the rows that pass the verifier's inlier test with it
    pub fn lf_mkd_match_guided_pairs_device(h: *mut lf_mkd, d_a: *const f32, d_kps_a: *const lf_mkd_keypoint,
                                            d_offsets_a: *const u64, na_total: u64, d_b: *const f32,
                                            d_kps_b: *const lf_mkd_keypoint, d_offsets_b: *const u64, nb_total: u64,
                                            d_model: *const f32, n_pairs: u32, kind: u32, threshold_px: f32, ratio: f32,
                                            flags: u32, d_match_ab: *mut i32, d_match_ba: *mut i32, d_best: *mut f32,
                                            d_second: *mut f32, stream: *mut c_void) -> c_int;
    pub fn lf_mkd_match(h: *mut lf_mkd, a: *const f32, na: u64, b: *const f32, nb: u64, ratio: f32,
                        matches: *mut i32) -> c_int;
    pub fn lf_mkd_match_overflowed(h: *mut lf_mkd, stream: *mut c_void, n_rows: *mut u64) -> c_int;

    // 8-bit descriptors: byte = clamp(rint(x * scale), -127, 127) + 128 (scale 0.0: the default, 256), and the matcher
    // over such rows, decided on exact integer similarities (d_best / d_second are i32)
    pub fn lf_mkd_quantize_descriptors_device(h: *mut lf_mkd, d_desc: *const f32, n: u64, scale: f32, d_q: *mut u8,
                                              stream: *mut c_void) -> c_int;
    pub fn lf_mkd_quantize_descriptors(h: *mut lf_mkd, desc: *const f32, n: u64, scale: f32, q: *mut u8) -> c_int;
    pub fn lf_mkd_match_q8_device(h: *mut lf_mkd, d_a: *const u8, na: u64, d_b: *const u8, nb: u64,
                                  d_exclude_lo: *const u32, d_exclude_hi: *const u32, ratio: f32, d_match: *mut i32,
                                  d_best: *mut i32, d_second: *mut i32, stream: *mut c_void) -> c_int;
    pub fn lf_mkd_match_q8(h: *mut lf_mkd, a: *const u8, na: u64, b: *const u8, nb: u64, ratio: f32,
                           matches: *mut i32) -> c_int;
    // the grid (a blocks x b splits) and the scratch lf_mkd_match_q8_device takes for a size; host only, no handle
    pub fn lf_mkd_match_q8_plan(na: u64, nb: u64, num_cus: u32, a_blocks: *mut u32, b_splits: *mut u32,
                                scratch_bytes: *mut u64) -> c_int;
    // each a row's k best b rows over 8-bit rows (1 <= k <= LF_MKD_KNN_MAX): d_index / d_score [na][k] i32, larger sum first,
    // among equal sums the higher index first; -1 / i32::MIN beyond the number of candidates; d_score / score may be null
    pub fn lf_mkd_knn_q8_device(h: *mut lf_mkd, d_a: *const u8, na: u64, d_b: *const u8, nb: u64,
                                d_exclude_lo: *const u32, d_exclude_hi: *const u32, k: u32, d_index: *mut i32,
                                d_score: *mut i32, stream: *mut c_void) -> c_int;
    pub fn lf_mkd_knn_q8(h: *mut lf_mkd, a: *const u8, na: u64, b: *const u8, nb: u64, k: u32, index: *mut i32,
                         score: *mut i32) -> c_int;
    // the grid (a blocks x b splits) and the scratch lf_mkd_knn_q8_device takes for a size and k; host only, no handle
    pub fn lf_mkd_knn_q8_plan(na: u64, nb: u64, k: u32, num_cus: u32, a_blocks: *mut u32, b_splits: *mut u32,
                              scratch_bytes: *mut u64) -> c_int;
    // the ratio test against the best neighbour from another group over 8-bit rows: d_group_of_b [nb] u32 (only equality is
    // used); d_best is the best score, d_rival the best score among the rows of another group than the best's (i32::MIN:
    // none); d_match is the best's index if ratio <= 0 or best * ratio > rival, else -1; d_best / d_rival may be null
    pub fn lf_mkd_match_q8_grouped_device(h: *mut lf_mkd, d_a: *const u8, na: u64, d_b: *const u8, nb: u64,
                                          d_group_of_b: *const u32, d_exclude_lo: *const u32, d_exclude_hi: *const u32,
                                          ratio: f32, d_match: *mut i32, d_best: *mut i32, d_rival: *mut i32,
                                          stream: *mut c_void) -> c_int;
    pub fn lf_mkd_match_q8_grouped(h: *mut lf_mkd, a: *const u8, na: u64, b: *const u8, nb: u64, group_of_b: *const u32,
                                   ratio: f32, matches: *mut i32, best: *mut i32, rival: *mut i32) -> c_int;
    // the grid (a blocks x b splits) and the scratch lf_mkd_match_q8_grouped_device takes for a size; host only, no handle
    pub fn lf_mkd_match_q8_grouped_plan(na: u64, nb: u64, num_cus: u32, a_blocks: *mut u32, b_splits: *mut u32,
                                        scratch_bytes: *mut u64) -> c_int;
    // d_votes [n_groups_a][n_groups_b] u32, zeroed and then counted: one vote per row with 0 <= d_match[i] < nb and both
    // group ids below their counts; d_group_of_a may be null (group 0)
    pub fn lf_mkd_vote_groups_device(h: *mut lf_mkd, d_match: *const i32, na: u64, d_group_of_a: *const u32, n_groups_a: u32,
                                     d_group_of_b: *const u32, nb: u64, n_groups_b: u32, d_votes: *mut u32,
                                     stream: *mut c_void) -> c_int;
    // n_pairs match problems over 8-bit rows in one launch: lf_mkd_match_pairs_device's layout (offsets on the device), each
    // pair decided as lf_mkd_match_q8_device decides it alone; d_best / d_second are i32; flags: LF_MKD_MATCH_MUTUAL
    pub fn lf_mkd_match_q8_pairs_device(h: *mut lf_mkd, d_a: *const u8, d_offsets_a: *const u64, na_total: u64,
                                        d_b: *const u8, d_offsets_b: *const u64, nb_total: u64, n_pairs: u32, ratio: f32,
                                        flags: u32, d_match_ab: *mut i32, d_match_ba: *mut i32, d_best: *mut i32,
                                        d_second: *mut i32, stream: *mut c_void) -> c_int;
    // that batch under each pair's verified model: lf_mkd_match_guided_pairs_device's keypoints, model, kind and threshold over
    // 8-bit rows, decided on the exact integer sums of the admissible rows; the grid is lf_mkd_match_q8_pairs_plan's
    pub fn lf_mkd_match_q8_guided_pairs_device(h: *mut lf_mkd, d_a: *const u8, d_kps_a: *const lf_mkd_keypoint,
                                               d_offsets_a: *const u64, na_total: u64, d_b: *const u8,
                                               d_kps_b: *const lf_mkd_keypoint, d_offsets_b: *const u64, nb_total: u64,
                                               d_model: *const f32, n_pairs: u32, kind: u32, threshold_px: f32, ratio: f32,
                                               flags: u32, d_match_ab: *mut i32, d_match_ba: *mut i32, d_best: *mut i32,
                                               d_second: *mut i32, stream: *mut c_void) -> c_int;
    // the a rows one workgroup of that launch owns and its grid, floor(rows / block_rows) + n_pairs per direction; host only
    pub fn lf_mkd_match_q8_pairs_plan(na_total: u64, nb_total: u64, n_pairs: u32, both_directions: u32,
                                      block_rows: *mut u32, workgroups: *mut u64) -> c_int;

    // edge lists over a pool (rows + image offsets): any pairs of images in one call, no row copied.  The edge layout of a side
    // is the pair layout whose pair e has the rows of that side's image of edge e; one call per side writes it
    pub fn lf_mkd_edge_layout_device(h: *mut lf_mkd, d_image_offsets: *const u64, n_images: u32, n_rows_total: u64,
                                     d_edge_image: *const u32, n_edges: u32, d_edge_offsets: *mut u64,
                                     stream: *mut c_void) -> c_int;
    // rows of row_bytes bytes (a multiple of 4 up to 512: keypoints 20, q8 rows 128, f32 rows 512) from the pool into the
    // edge layout
    pub fn lf_mkd_gather_edge_rows_device(h: *mut lf_mkd, d_src: *const c_void, row_bytes: u32, d_image_offsets: *const u64,
                                          n_images: u32, n_rows_total: u64, d_edge_image: *const u32,
                                          d_edge_offsets: *const u64, capacity_rows: u64, n_edges: u32, d_dst: *mut c_void,
                                          stream: *mut c_void) -> c_int;
    // edge e = image d_edge_a[e] of pool a against image d_edge_b[e] of pool b, decided as lf_mkd_match_q8_device decides the
    // two images alone; outputs in the edge layouts; the grid is lf_mkd_match_q8_pairs_plan's over the capacities
    pub fn lf_mkd_match_q8_edges_device(h: *mut lf_mkd, d_a: *const u8, d_image_offsets_a: *const u64, n_images_a: u32,
                                        na_total: u64, d_b: *const u8, d_image_offsets_b: *const u64, n_images_b: u32,
                                        nb_total: u64, d_edge_a: *const u32, d_edge_b: *const u32,
                                        d_edge_offsets_a: *const u64, ea_capacity: u64, d_edge_offsets_b: *const u64,
                                        eb_capacity: u64, n_edges: u32, ratio: f32, flags: u32, d_match_ab: *mut i32,
                                        d_match_ba: *mut i32, d_best: *mut i32, d_second: *mut i32,
                                        stream: *mut c_void) -> c_int;
    // tracks: d_track [n_rows_total] = the smallest pool row of every row's connected component under the links d_match holds
    // in the a side's edge layout; d_track_len / d_track_dup (nullable) per label the track's rows and its conflicting rows;
    // flags: LF_MKD_TRACKS_ACCUMULATE
    pub fn lf_mkd_build_tracks_device(h: *mut lf_mkd, d_image_offsets: *const u64, n_images: u32, n_rows_total: u64,
                                      d_edge_a: *const u32, d_edge_b: *const u32, d_edge_offsets_a: *const u64,
                                      ea_capacity: u64, n_edges: u32, d_match: *const i32, flags: u32, d_track: *mut i32,
                                      d_track_len: *mut u32, d_track_dup: *mut u32, stream: *mut c_void) -> c_int;
    // track tables: the CSR table of the tracks lf_mkd_build_tracks_device labelled (d_track_offsets [track_capacity + 1],
    // d_obs_row / d_obs_image [obs_capacity], d_row_track [n_rows_total], d_counts [4] = {T, O, selected, wanted observations});
    // flags: LF_MKD_TRACK_TABLE_CONSISTENT; the plan is host only; the gather copies src row d_obs_row[k] to dst row k
    pub fn lf_mkd_track_table_plan(n_rows_total: u64, min_len: u32, key_bits: *mut u32, passes: *mut u32, block_rows: *mut u32,
                                   scratch_bytes: *mut u64) -> c_int;
    pub fn lf_mkd_track_table_device(h: *mut lf_mkd, d_image_offsets: *const u64, n_images: u32, n_rows_total: u64,
                                     d_track: *const i32, d_track_len: *const u32, d_track_dup: *const u32, min_len: u32,
                                     flags: u32, track_capacity: u64, obs_capacity: u64, d_track_offsets: *mut u64,
                                     d_obs_row: *mut i32, d_obs_image: *mut u32, d_row_track: *mut i32, d_counts: *mut u32,
                                     stream: *mut c_void) -> c_int;
    pub fn lf_mkd_gather_track_rows_device(h: *mut lf_mkd, d_src: *const c_void, row_bytes: u32, n_rows_total: u64,
                                           d_obs_row: *const i32, d_counts: *const u32, obs_capacity: u64, d_dst: *mut c_void,
                                           stream: *mut c_void) -> c_int;
    // link tables: the CSR table of the links d_match holds in the a side's edge layout (d_link_offsets [n_edges + 1],
    // d_link_a / d_link_b / d_link_edge [link_capacity], d_edge_links [n_edges], d_match_kept like d_match, d_counts [4] =
    // {kept edges, O, selected edges, wanted links}); flags: LF_MKD_LINK_TABLE_LOCAL; the plan is host only
    pub fn lf_mkd_link_table_plan(ea_capacity: u64, n_edges: u32, slot_entries: *mut u32, slots: *mut u64,
                                  scan_fanout: *mut u32, scan_levels: *mut u32, scratch_bytes: *mut u64) -> c_int;
    pub fn lf_mkd_link_table_device(h: *mut lf_mkd, d_image_offsets: *const u64, n_images: u32, n_rows_total: u64,
                                    d_edge_a: *const u32, d_edge_b: *const u32, d_edge_offsets_a: *const u64,
                                    ea_capacity: u64, n_edges: u32, d_match: *const i32, min_links: u32, flags: u32,
                                    link_capacity: u64, d_link_offsets: *mut u64, d_link_a: *mut i32, d_link_b: *mut i32,
                                    d_link_edge: *mut u32, d_edge_links: *mut u32, d_match_kept: *mut i32,
                                    d_counts: *mut u32, stream: *mut c_void) -> c_int;
    // candidate edges: per row of d_votes [n_a][n_b] its k best columns (larger votes first, among equal ones the LOWER
    // column: d_rank / d_rank_votes [n_a][k], nullable) and the edges those picks make (d_edge_a / d_edge_b / d_edge_votes
    // [edge_capacity], 0xFFFFFFFF behind the edges; d_counts [4] = {kept edges, edges, picks, rows with a pick}); flags:
    // LF_MKD_SELECT_SKIP_SELF, LF_MKD_SELECT_UNIQUE; k <= LF_MKD_SELECT_MAX_K; the plan is host only
    pub fn lf_mkd_select_edges_plan(n_a: u32, n_b: u32, k: u32, edge_capacity: u64, flags: u32, compiled_k: *mut u32,
                                    rows_per_workgroup: *mut u32, workgroups: *mut u64, launches: *mut u32,
                                    scratch_bytes: *mut u64) -> c_int;
    pub fn lf_mkd_select_edges_device(h: *mut lf_mkd, d_votes: *const u32, n_a: u32, n_b: u32, k: u32, min_votes: u32,
                                      flags: u32, edge_capacity: u64, d_rank: *mut i32, d_rank_votes: *mut u32,
                                      d_edge_a: *mut u32, d_edge_b: *mut u32, d_edge_votes: *mut u32, d_counts: *mut u32,
                                      stream: *mut c_void) -> c_int;
    // covisibility tables: d_covis [n_images][n_images] = per pair of images the tracks of a track table (d_track_offsets
    // [track_capacity + 1], d_obs_image [obs_capacity], d_table_counts: lf_mkd_track_table_device's outputs) that both see,
    // the diagonal the tracks an image sees; the pairs d_edge_a / d_edge_b [n_edges] (nullable) name are set to 0; flags:
    // LF_MKD_COVIS_ACCUMULATE; the plan is host only
    pub fn lf_mkd_covisibility_plan(n_images: u32, track_capacity: u64, obs_capacity: u64, n_edges: u64, flags: u32,
                                    form: *mut u32, workgroups: *mut u64, launches: *mut u32, scratch_bytes: *mut u64) -> c_int;
    pub fn lf_mkd_covisibility_device(h: *mut lf_mkd, d_track_offsets: *const u64, track_capacity: u64, d_obs_image: *const u32,
                                      obs_capacity: u64, d_table_counts: *const u32, n_images: u32, d_edge_a: *const u32,
                                      d_edge_b: *const u32, n_edges: u64, flags: u32, d_covis: *mut u32,
                                      stream: *mut c_void) -> c_int;
    // two-view poses: per edge R [9], t [3] (x_b = R x_a + t, |t| = 1), stats [4], optional sigma [3] and per link optional
    // points [4], from d_F [n_edges][9], d_intrinsics [n_images][4] (fx, fy, cx, cy) and a link table of pool rows; flags: 0;
    // the host form takes one pair and a match array and returns points per row of a
    pub fn lf_mkd_two_view_pose_device(h: *mut lf_mkd, d_kps: *const lf_mkd_keypoint, n_rows_total: u64, d_edge_a: *const u32,
                                       d_edge_b: *const u32, n_edges: u32, d_intrinsics: *const f32, n_images: u32,
                                       d_f: *const f32, d_link_offsets: *const u64, d_link_a: *const i32, d_link_b: *const i32,
                                       link_capacity: u64, min_parallax_deg: f32, flags: u32, d_r: *mut f32, d_t: *mut f32,
                                       d_stats: *mut u32, d_sigma: *mut f32, d_points: *mut f32, stream: *mut c_void) -> c_int;
    pub fn lf_mkd_two_view_pose(h: *mut lf_mkd, fundamental: *const f32, k_a: *const f32, k_b: *const f32,
                                kps_a: *const lf_mkd_keypoint, na: u64, kps_b: *const lf_mkd_keypoint, nb: u64,
                                matches: *const i32, min_parallax_deg: f32, flags: u32, r: *mut f32, t: *mut f32,
                                stats: *mut u32, sigma: *mut f32, points: *mut f32) -> c_int;
    // track triangulation: per track of a track table points [4] (X, Y, Z, the parallax cosine), stats [4], optional err [2]
    // and per observation an optional state, from d_intrinsics [n_images][4] and d_poses [n_images][12] (R row-major, then t;
    // world to camera); flags: 0; the host form takes host arrays, n_tracks and n_obs
    pub fn lf_mkd_triangulate_tracks_device(h: *mut lf_mkd, d_kps: *const lf_mkd_keypoint, n_rows_total: u64,
                                            d_track_offsets: *const u64, track_capacity: u64, d_obs_row: *const i32,
                                            d_obs_image: *const u32, obs_capacity: u64, d_table_counts: *const u32,
                                            d_intrinsics: *const f32, d_poses: *const f32, n_images: u32, max_reproj_px: f32,
                                            rounds: u32, flags: u32, d_points: *mut f32, d_stats: *mut u32, d_err: *mut f32,
                                            d_obs_state: *mut u32, stream: *mut c_void) -> c_int;
    pub fn lf_mkd_triangulate_tracks(h: *mut lf_mkd, kps: *const lf_mkd_keypoint, n_rows_total: u64, track_offsets: *const u64,
                                     n_tracks: u64, obs_row: *const i32, obs_image: *const u32, n_obs: u64,
                                     intrinsics: *const f32, poses: *const f32, n_images: u32, max_reproj_px: f32, rounds: u32,
                                     flags: u32, points: *mut f32, stats: *mut u32, err: *mut f32,
                                     obs_state: *mut u32) -> c_int;
    // camera resection: per image that is not registered (an all-zero R in d_poses [n_images][12]; every image with
    // LF_MKD_RESECT_ALL = 1) its pose from the keypoints it owns in tracks with a point: poses_out [12] (may be d_poses), stats
    // [4], optional err [2] and per row an optional state; the host form takes ONE image's host arrays
    pub fn lf_mkd_resect_cameras_device(h: *mut lf_mkd, d_kps: *const lf_mkd_keypoint, d_image_offsets: *const u64, n_images: u32,
                                        n_rows_total: u64, d_row_track: *const i32, d_points: *const f32, track_capacity: u64,
                                        d_table_counts: *const u32, d_intrinsics: *const f32, d_poses: *const f32,
                                        max_reproj_px: f32, min_parallax_deg: f32, n_samples: u32, min_inliers: u32, rounds: u32,
                                        seed: u32, flags: u32, d_poses_out: *mut f32, d_stats: *mut u32, d_err: *mut f32,
                                        d_row_state: *mut u32, stream: *mut c_void) -> c_int;
    pub fn lf_mkd_resect_camera(h: *mut lf_mkd, kps: *const lf_mkd_keypoint, n_rows: u64, row_track: *const i32,
                                points: *const f32, n_tracks: u64, intrinsics: *const f32, max_reproj_px: f32,
                                min_parallax_deg: f32, n_samples: u32, min_inliers: u32, rounds: u32, seed: u32, flags: u32,
                                pose: *mut f32, stats: *mut u32, err: *mut f32, row_state: *mut u32) -> c_int;
    // track descriptors: per track of a track table one 8-bit row [128], the sum of its observations' pool rows normalised and
    // quantised again (an optional state filter per observation, an optional point filter per track; zero rows, all bytes 128,
    // elsewhere and up to track_capacity), optional desc_stats [2] = contributors, smallest similarity; lf_mkd_match_q8_device
    // against the rows gives the d_row_track resection reads; the host form takes host arrays, n_tracks and n_obs
    pub fn lf_mkd_track_descriptors_device(h: *mut lf_mkd, d_q: *const u8, n_rows_total: u64, d_track_offsets: *const u64,
                                           track_capacity: u64, d_obs_row: *const i32, obs_capacity: u64,
                                           d_table_counts: *const u32, d_obs_state: *const u32, min_state: u32,
                                           d_points: *const f32, min_parallax_deg: f32, scale: f32, d_desc: *mut u8,
                                           d_desc_stats: *mut i32, stream: *mut c_void) -> c_int;
    pub fn lf_mkd_track_descriptors(h: *mut lf_mkd, q: *const u8, n_rows_total: u64, track_offsets: *const u64, n_tracks: u64,
                                    obs_row: *const i32, n_obs: u64, obs_state: *const u32, min_state: u32, points: *const f32,
                                    min_parallax_deg: f32, scale: f32, desc: *mut u8, desc_stats: *mut i32) -> c_int;
    // bundle adjustment: Levenberg-Marquardt over the free cameras (registered, not marked in d_camera_fixed) and the free
    // points of a track table, the reduced camera system by preconditioned conjugate gradients: poses_out [n_images][12] (may
    // be d_poses), points_out [track_capacity][4] (may be d_points), an optional state per observation, trace f64
    // [iterations][8], counts [4]; the host form takes host arrays with T = n_tracks and O = n_obs
    pub fn lf_mkd_bundle_adjust_device(h: *mut lf_mkd, d_kps: *const lf_mkd_keypoint, d_image_offsets: *const u64, n_images: u32,
                                       n_rows_total: u64, d_track_offsets: *const u64, track_capacity: u64,
                                       d_obs_row: *const i32, d_obs_image: *const u32, obs_capacity: u64,
                                       d_table_counts: *const u32, d_points: *const f32, d_intrinsics: *const f32,
                                       d_poses: *const f32, d_obs_state: *const u32, d_camera_fixed: *const u32,
                                       max_reproj_px: f32, lambda0: f32, iterations: u32, cg_iterations: u32, cg_tol: f32,
                                       flags: u32, d_poses_out: *mut f32, d_points_out: *mut f32, d_obs_state_out: *mut u32,
                                       d_trace: *mut f64, d_counts: *mut u32, stream: *mut c_void) -> c_int;
    pub fn lf_mkd_bundle_adjust(h: *mut lf_mkd, kps: *const lf_mkd_keypoint, image_offsets: *const u64, n_images: u32,
                                n_rows_total: u64, track_offsets: *const u64, n_tracks: u64, obs_row: *const i32,
                                obs_image: *const u32, n_obs: u64, points: *const f32, intrinsics: *const f32,
                                poses: *const f32, obs_state: *const u32, camera_fixed: *const u32, max_reproj_px: f32,
                                lambda0: f32, iterations: u32, cg_iterations: u32, cg_tol: f32, flags: u32,
                                poses_out: *mut f32, points_out: *mut f32, obs_state_out: *mut u32, trace: *mut f64,
                                counts: *mut u32) -> c_int;
    // the same with the intrinsics of the images that share a lens refined: d_camera_group [n_images] (nullable: one group),
    // refine = LF_MKD_BA_REFINE_FOCAL (1) | LF_MKD_BA_REFINE_PRINCIPAL (2); intrinsics_out [n_images][4] (may be d_intrinsics),
    // an optional group_out [n_groups][3] = (s, dx, dy), trace f64 [iterations][9], counts [5]
    pub fn lf_mkd_bundle_adjust_intrinsics_device(h: *mut lf_mkd, d_kps: *const lf_mkd_keypoint, d_image_offsets: *const u64,
                                                  n_images: u32, n_rows_total: u64, d_track_offsets: *const u64,
                                                  track_capacity: u64, d_obs_row: *const i32, d_obs_image: *const u32,
                                                  obs_capacity: u64, d_table_counts: *const u32, d_points: *const f32,
                                                  d_intrinsics: *const f32, d_poses: *const f32, d_obs_state: *const u32,
                                                  d_camera_fixed: *const u32, d_camera_group: *const u32, n_groups: u32,
                                                  refine: u32, max_reproj_px: f32, lambda0: f32, iterations: u32,
                                                  cg_iterations: u32, cg_tol: f32, flags: u32, d_poses_out: *mut f32,
                                                  d_points_out: *mut f32, d_intrinsics_out: *mut f32, d_group_out: *mut f32,
                                                  d_obs_state_out: *mut u32, d_trace: *mut f64, d_counts: *mut u32,
                                                  stream: *mut c_void) -> c_int;
    pub fn lf_mkd_bundle_adjust_intrinsics(h: *mut lf_mkd, kps: *const lf_mkd_keypoint, image_offsets: *const u64, n_images: u32,
                                           n_rows_total: u64, track_offsets: *const u64, n_tracks: u64, obs_row: *const i32,
                                           obs_image: *const u32, n_obs: u64, points: *const f32, intrinsics: *const f32,
                                           poses: *const f32, obs_state: *const u32, camera_fixed: *const u32,
                                           camera_group: *const u32, n_groups: u32, refine: u32, max_reproj_px: f32,
                                           lambda0: f32, iterations: u32, cg_iterations: u32, cg_tol: f32, flags: u32,
                                           poses_out: *mut f32, points_out: *mut f32, intrinsics_out: *mut f32,
                                           group_out: *mut f32, obs_state_out: *mut u32, trace: *mut f64,
                                           counts: *mut u32) -> c_int;
    // view-graph checks: the triangle vote over the posed edges (R [n_edges][9] and stats [n_edges][4] of the pose call), global
    // rotations [n_images][9] by a tree and quaternion averaging over the kept edges, edge stats [4], an optional residual, image
    // stats [4], an optional filtered match array (may be d_match), counts [8]; flags = LF_MKD_VIEW_GRAPH_USE_UNCHECKED (1),
    // root = an image id or 0xFFFFFFFF; the plan needs no device; the host form takes host arrays
    pub fn lf_mkd_view_graph_plan(n_images: u32, n_edges: u32, tree_rounds: u32, iterations: u32, flags: u32, with_match: u32,
                                  launches: *mut u32, scratch_bytes: *mut u64, form: *mut u32) -> c_int;
    pub fn lf_mkd_view_graph_device(h: *mut lf_mkd, d_edge_a: *const u32, d_edge_b: *const u32, n_edges: u32, d_R: *const f32,
                                    d_pose_stats: *const u32, n_images: u32, max_loop_deg: f32, min_front: u32, root: u32,
                                    tree_rounds: u32, iterations: u32, flags: u32, d_edge_offsets_a: *const u64,
                                    ea_capacity: u64, d_match: *const i32, d_match_out: *mut i32, d_rotations: *mut f32,
                                    d_edge_stats: *mut u32, d_edge_residual: *mut f32, d_image_stats: *mut u32,
                                    d_counts: *mut u32, stream: *mut c_void) -> c_int;
    pub fn lf_mkd_view_graph(h: *mut lf_mkd, edge_a: *const u32, edge_b: *const u32, n_edges: u32, R: *const f32,
                             pose_stats: *const u32, n_images: u32, max_loop_deg: f32, min_front: u32, root: u32,
                             tree_rounds: u32, iterations: u32, flags: u32, edge_offsets_a: *const u64, n_entries: u64,
                             matches: *const i32, match_out: *mut i32, rotations: *mut f32, edge_stats: *mut u32,
                             edge_residual: *mut f32, image_stats: *mut u32, counts: *mut u32) -> c_int;
    // initial poses [n_images][12] from the view graph's rotations, its tree (image_stats) and the tree edges' translations
    pub fn lf_mkd_tree_poses_device(h: *mut lf_mkd, d_edge_a: *const u32, d_edge_b: *const u32, d_t: *const f32, n_edges: u32,
                                    d_rotations: *const f32, d_image_stats: *const u32, n_images: u32, max_depth: u32,
                                    d_poses: *mut f32, stream: *mut c_void) -> c_int;
    pub fn lf_mkd_tree_poses(h: *mut lf_mkd, edge_a: *const u32, edge_b: *const u32, t: *const f32, n_edges: u32,
                             rotations: *const f32, image_stats: *const u32, n_images: u32, max_depth: u32,
                             poses: *mut f32) -> c_int;
    // global positions: all camera centres and track points at once under held rotations -- poses_out (may be poses), optional
    // points [4], observation states and trace f64 [sweeps][4], image stats [4], counts [8]; the plan needs no device
    pub fn lf_mkd_global_positions_plan(n_images: u32, track_capacity: u64, sweeps: u32, launches: *mut u32,
                                        scratch_bytes: *mut u64) -> c_int;
    pub fn lf_mkd_global_positions_device(h: *mut lf_mkd, d_kps: *const lf_mkd_keypoint, d_image_offsets: *const u64,
                                          n_images: u32, n_rows_total: u64, d_track_offsets: *const u64, track_capacity: u64,
                                          d_obs_row: *const i32, d_obs_image: *const u32, obs_capacity: u64,
                                          d_table_counts: *const u32, d_row_track: *const i32, d_intrinsics: *const f32,
                                          d_poses: *const f32, sweeps: u32, warm: u32, robust_deg: f32, min_obs: u32, flags: u32,
                                          d_poses_out: *mut f32, d_points_out: *mut f32, d_obs_state: *mut u32,
                                          d_image_stats: *mut u32, d_trace: *mut f64, d_counts: *mut u32,
                                          stream: *mut c_void) -> c_int;
    pub fn lf_mkd_global_positions(h: *mut lf_mkd, kps: *const lf_mkd_keypoint, image_offsets: *const u64, n_images: u32,
                                   n_rows_total: u64, track_offsets: *const u64, n_tracks: u64, obs_row: *const i32,
                                   obs_image: *const u32, n_obs: u64, row_track: *const i32, intrinsics: *const f32,
                                   poses: *const f32, sweeps: u32, warm: u32, robust_deg: f32, min_obs: u32, flags: u32,
                                   poses_out: *mut f32, points_out: *mut f32, obs_state: *mut u32, image_stats: *mut u32,
                                   trace: *mut f64, counts: *mut u32) -> c_int;

    // RANSAC homography verification of matches: one pair from host memory, or n_pairs pairs on the device in one call
    pub fn lf_mkd_verify_homography(h: *mut lf_mkd, kps_a: *const lf_mkd_keypoint, na: u64, kps_b: *const lf_mkd_keypoint,
                                    nb: u64, matches: *const i32, n_hypotheses: u32, threshold_px: f32, seed: u32, flags: u32,
                                    homography: *mut f32, verified: *mut i32, stats: *mut u32) -> c_int;
    pub fn lf_mkd_verify_homography_device(h: *mut lf_mkd, d_kps_a: *const lf_mkd_keypoint, d_offsets_a: *const u64,
                                           d_kps_b: *const lf_mkd_keypoint, d_offsets_b: *const u64, d_match: *const i32,
                                           n_pairs: u32, n_hypotheses: u32, threshold_px: f32, seed: u32, flags: u32,
                                           d_homography: *mut f32, d_verified: *mut i32, d_stats: *mut u32,
                                           stream: *mut c_void) -> c_int;
    // RANSAC fundamental-matrix verification (7-point samples, Sampson distance): the same two faces
    pub fn lf_mkd_verify_fundamental(h: *mut lf_mkd, kps_a: *const lf_mkd_keypoint, na: u64, kps_b: *const lf_mkd_keypoint,
                                     nb: u64, matches: *const i32, n_hypotheses: u32, threshold_px: f32, seed: u32, flags: u32,
                                     fundamental: *mut f32, verified: *mut i32, stats: *mut u32) -> c_int;
    pub fn lf_mkd_verify_fundamental_device(h: *mut lf_mkd, d_kps_a: *const lf_mkd_keypoint, d_offsets_a: *const u64,
                                            d_kps_b: *const lf_mkd_keypoint, d_offsets_b: *const u64, d_match: *const i32,
                                            n_pairs: u32, n_hypotheses: u32, threshold_px: f32, seed: u32, flags: u32,
                                            d_fundamental: *mut f32, d_verified: *mut i32, d_stats: *mut u32,
                                            stream: *mut c_void) -> c_int;

    // the path's one collective: the all-gather of descriptor shards over RCCL (configs[3])
    pub fn lf_mkd_comm_unique_id(id: *mut u8) -> c_int;
    pub fn lf_mkd_comm_create(h: *mut lf_mkd, id: *const u8, n_ranks: i32, rank: i32, out: *mut *mut lf_mkd_comm) -> c_int;
    pub fn lf_mkd_comm_destroy(c: *mut lf_mkd_comm) -> c_int;
    pub fn lf_mkd_comm_info(c: *const lf_mkd_comm, rccl_version: *mut i32, n_ranks: *mut i32, rank: *mut i32) -> c_int;
    pub fn lf_mkd_allgather_descriptors(h: *mut lf_mkd, c: *mut lf_mkd_comm, counts: *const u64, d_buf: *mut f32,
                                        mode: i32, stream: *mut c_void) -> c_int;
    pub fn lf_mkd_plan_upload(width: u32, height: u32, bytes_per_pixel: u32, n_scales: u32, cuts: *mut u32, max_cuts: u32,
                              n_cuts: *mut u32, modelled_us: *mut f64, one_piece_us: *mut f64) -> c_int;
    pub fn lf_mkd_comm_loopback(h: *mut lf_mkd, c: *mut lf_mkd_comm, d_src: *const f32, d_dst: *mut f32, n_rows: u64,
                                stream: *mut c_void) -> c_int;
    pub fn lf_mkd_comm_last_form(c: *const lf_mkd_comm) -> c_int;

    pub fn lf_mkd_get_coarse_layer(h: *mut lf_mkd, layer: u32, out: *mut f32) -> c_int;
    pub fn lf_mkd_sample_patches_device(h: *mut lf_mkd, d_kps: *const lf_mkd_keypoint, n: u64, d_patches: *mut f32,
                                        stream: *mut c_void) -> c_int;
    pub fn lf_mkd_get_pyramid_level(h: *mut lf_mkd, level: u32, out: *mut f32, w: *mut u32, hgt: *mut u32) -> c_int;
    pub fn lf_mkd_get_pyramid_level_apron(h: *mut lf_mkd, level: u32, out: *mut f32, w: *mut u32, hgt: *mut u32,
                                          apron: *mut u32) -> c_int;
    pub fn lf_mkd_build_constants(mean: *const f32, eigvals: *const f32, eigvecs: *const f32,
                                  gradient_angle: *mut f32, embedding_polar: *mut f32,
                                  embedding_cartesian: *mut f32, w_t: *mut f32) -> c_int;
    pub fn lf_mkd_kernel_times(h: *mut lf_mkd, pool_ms: *mut f64, whiten_ms: *mut f64, launches: *mut u64) -> c_int;
    pub fn lf_mkd_kernel_clock(h: *mut lf_mkd, stream: *mut c_void, shader_mhz: *mut f64, kernel_ms: *mut f64) -> c_int;
    pub fn lf_mkd_detect_recordings(h: *const lf_mkd, n_recordings: *mut u32, n_banded: *mut u32, n_sightings: *mut u32) -> c_int;
    pub fn lf_mkd_synchronize(h: *mut lf_mkd) -> c_int;
    pub fn lf_mkd_version() -> *const c_char;
}
