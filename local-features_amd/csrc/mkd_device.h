// Launch interface between the C ABI (lf_mkd.cpp, lf_mkd_match.cpp, lf_mkd_tables.cpp, lf_mkd_geometry.cpp) and the gfx950 kernels
// (mkd_describe.hip, mkd_pyramid.hip, mkd_orient.hip, mkd_detect.hip; the matchers mkd_match.hip, mkd_match_q8.hip,
// mkd_match_q8_knn.hip, mkd_match_q8_grouped.hip, mkd_match_guided.hip, mkd_match_q8_guided.hip, mkd_match_q8_edges.hip; the
// tables mkd_tracks.hip, mkd_track_table.hip, mkd_link_table.hip, mkd_select_edges.hip, mkd_covisibility.hip; the geometry
// mkd_verify.hip, mkd_two_view_pose.hip, mkd_triangulate.hip, mkd_resect.hip, mkd_bundle.hip, mkd_view_graph.hip,
// mkd_positions.hip).  The scene struct the reconstruction launchers take is mkd_scene.h's, which the files that fill or read
// it include themselves, behind their arithmetic headers.
#pragma once
#include <hip/hip_runtime.h>

#include <functional>
#include <stdint.h>

#include "mkd_verify_pair.h"

#define LF_ANGLE_SHADER 0
#define LF_ANGLE_EXACT 1
#define LF_ANGLE_EXACT_ZERO 2   // exact direction, but angle 0 where gx == 0 like the shader
#define LF_POOL_F16X3 1         // = LF_MKD_POOL_F16X3 (lf_mkd.h); the ABI's 0 ("default") is mapped to it at creation
#define LF_POOL_F32 2           // = LF_MKD_POOL_F32
#define LF_POOL_F16_FP6 3       // = LF_MKD_POOL_F16_FP6

namespace lfmkd {

typedef float f32x4 __attribute__((ext_vector_type(4)));
struct SceneTables;   // mkd_scene.h

constexpr int kMaxPyrLevels = 16;

// Patch pyramid: levels packed back to back in one allocation; level l is w[l] x h[l] f32, rows pitch[l] floats apart.
// Every level carries an APRON of kPyrApron texels on every side, filled with the level's own texels under MirroredRepeat
// (mod.rs:940-943): a keypoint whose centre lies inside its level reaches at most 22.7 rem + 2 < 48 texels from it
// (rem < 2), so its whole footprint is addressed without any mirror arithmetic.  offset[l] is texel (0, 0).  (Level 0 is also
// a-trous layer 0 of the detector and the orientation stage: they read it with its pitch.)
constexpr int kPyrApron = 48;
struct PyramidDesc {
    int levels;
    int w[kMaxPyrLevels], h[kMaxPyrLevels];
    int pitch[kMaxPyrLevels];    // floats between rows
    int apron[kMaxPyrLevels];    // mirrored texels around the level
    long offset[kMaxPyrLevels];  // in floats, of texel (0, 0)
};

// Row bands (lf_mkd_detect's upload / compute overlap; two pieces in round 5, any number since round 6): the frame reaches the
// device in pieces, and the row-tiled kernels of the pipeline's front -- level 0, the a-trous layers, the extremum scan -- run
// once per piece on the rows that piece completes, while the next piece is still on its way over PCIe.  A launch sequence is
// given the rows [lo, hi) of every stage it is to produce: hi = what the frame's rows so far allow (plan_row_bands: level 0
// needs two raw rows below an output row, a-trous layer l + 1 with dilation d = 2^l needs 2 d rows of layer l, the scan one row
// of every layer below a tile's candidates), lo = the previous piece's hi.  The last piece has hi = everything and also runs
// what is not row-tiled.  Splits fall on multiples of 12 rows for level 0, of d rows for a layer of dilation d, of a tile row
// (8 candidate rows) for the scan; no piece reads a row a later piece produces.
struct RowBands {
    int last;             // 1: the final piece -- every stage to its end, then the rest of the pipeline
    int level0_lo, level0_hi;       // pyramid level 0 = a-trous layer 0: rows (multiples of 12; hi of the last piece: the height)
    int layer_lo[8], layer_hi[8];   // a-trous layer l + 1 (dilation 2^l): rows (multiples of 2^l)
    int scan_lo, scan_hi;           // extremum scan: tile rows (8 candidate rows each)
};
// the `hi` fields for a frame of which the first raw_rows rows have arrived (`lo` and `last` are the caller's); false: the
// frame's shape does not take row bands (the staged kernels' alignment), or raw_rows covers the frame
bool plan_row_bands(int raw_rows, int w, int h, int n_layers, int border, RowBands &bands);

// Device copies of HostConsts' device layouts (mkd_consts.hpp).
struct DeviceConsts {
    short *colmap = nullptr;        // [336]
    float *pool_b_f32 = nullptr;    // [32][12][2][64][4]
    uint16_t *pool_b_f16 = nullptr; // [32][12][2][64][8]
    uint16_t *white_a_f16 = nullptr; // [11][8][2][64][8]
    float *white_a_f32 = nullptr;    // [21][4][8][64]
    // LF_MKD_POOL_F16_FP6 alone (the unfolded row form; null in the other modes)
    short *colmap_unfolded = nullptr;         // [336]
    uint16_t *pool_b_fp6 = nullptr;           // [32][15][2][64][8]
    uint16_t *white_a_f16_unfolded = nullptr; // [11][8][2][64][8]
    float *white_bias = nullptr;     // [128]  -W mean
    float *odd_cart = nullptr;       // [16] odd_cart_fx, then [32][4] odd_cart_gy (LF_MKD_POOL_F16X3's x-odd cartesian columns)
};

// patches [n][32][32] -> out [n][128] (and, when raw_out != nullptr, the un-whitened [n][238])
// (n_dev != nullptr: the count is read on the device, n only sizes the grid; same for the launchers below)
// waves: 0 = choose by size (4-wave workgroups when the request fits one round of them, else 8-wave), 4 / 8 = that form
void launch_describe(const float *patches, long n, const unsigned long long *n_dev, const DeviceConsts &dc,
                     int angle_mode, int pool_mode, float *out, float *raw_out, int num_cus, hipStream_t stream,
                     int waves = 0, unsigned long long *clk = nullptr, unsigned *claim = nullptr);
// clk (nullable, device, 4 words): workgroup 0 leaves (shader clock, 100 MHz clock) on entry and on exit
// claim (nullable, device, one word no other launch in flight uses): an 8-wave launch of at least kClaimRounds whole batches
// per workgroup clears it on `stream` and deals its batches at run time (mkd_pool); every other launch leaves it alone
constexpr long kClaimRounds = 4;
// frame_of_kp == nullptr: every keypoint belongs to frame 0
// (frame indices beyond n_frames - 1 -- caller's data -- are clamped to it: never a read outside the pyramid store)
void launch_sample_patches(const float *pyr, long pyr_stride, const PyramidDesc &pd, const float *kps,
                           const unsigned *frame_of_kp, unsigned n_frames, long n, const unsigned long long *n_dev, float psf,
                           float *patches, hipStream_t stream);
// keypoint mode in ONE launch (csrc/mkd_describe.hip): patches are sampled by producer waves of the describe workgroup
// straight into its LDS row ring and never touch HBM.  f16x3 pooling only.
void launch_describe_keypoints(const float *pyr, long pyr_stride, const PyramidDesc &pd, const float *kps,
                               const unsigned *frame_of_kp, unsigned n_frames, long n, const unsigned long long *n_dev,
                               float psf, const DeviceConsts &dc, int angle_mode, float *out, int num_cus, hipStream_t stream,
                               unsigned long long *clk = nullptr, float *xchg = nullptr, unsigned *xchg_words = nullptr,
                               long form_n = 0);
// form_n (0: n): the request size the choice between the whole-patch and the row-split forms follows, when it is not n
// xchg / xchg_words (nullable: the whole-patch forms only): scratch of the row-split form a request of at most 16 x CUs
// keypoints takes -- kp_split_exchange_bytes(num_cus) bytes and kp_split_counter_words(num_cus) u32 words, the words zero
// before the first launch (they return to zero at the end of every launch; word 0 counts partial sums that never arrived)
size_t kp_split_exchange_bytes(int num_cus);
size_t kp_split_counter_words(int num_cus);
// rest_stream (nullable): levels >= 1 are built there -- after `fork`, recorded on `stream` once level 0 and a-trous layer 1
// exist -- and `join` is recorded behind them; the caller waits for `join` before it samples patches
void launch_build_pyramid(const float *image, long image_stride, float *pyr, long pyr_stride, float *tmp_a,
                          float *tmp_b, const PyramidDesc &pd, int frames, float *layer1, long layer1_stride,
                          hipStream_t stream, hipStream_t rest_stream = nullptr, hipEvent_t fork = nullptr,
                          hipEvent_t join = nullptr, const std::function<void()> &main_next = {},
                          const unsigned char *image_u8 = nullptr, const RowBands *bands = nullptr);
// (image_u8 != nullptr: the frames are 8-bit luma, image_stride BYTES apart, `image` is ignored; a pixel is (float)v / 255.0f)

// a-trous layers 1 .. n_layers-1 over layer0 (= pyramid level 0); tmp holds frames x w x h floats
void launch_build_coarse_stack(const float *layer0, long layer0_stride, int layer0_pitch, float *coarse, long coarse_stride,
                               long layer_stride, float *tmp, int n_layers, int first_layer, int w, int h, int frames,
                               hipStream_t stream, const RowBands *bands = nullptr);
// extrema [n][4] -> kps [<= max_out][5] ordered by extremum then bin; angles [n][18], counts [n], sums [n/1024+1]
// are scratch (sums may be null for n <= 8192);
// totals[0] = written, totals[1] = dropped
void launch_orient(const float *layer0, long layer0_stride, int layer0_pitch, const float *coarse, long coarse_stride, long layer_stride,
                   int n_layers, int w, int h, const float *extrema, const unsigned *frame_of, long n,
                   const unsigned long long *n_dev, float *angles, unsigned *counts, unsigned *sums, float *kps,
                   unsigned *frame_of_kp, unsigned long long max_out, unsigned long long *totals, hipStream_t stream);

// cubes of the extremum scan for a w x h frame with n_fine DoG layers (tasks_detect.rs:300-310)
void scan_grid(int w, int h, int n_fine, int border, int skip_layers, int &gx, int &gy, int &gz);
// a-trous stack -> extrema [<= max_out][4] of all frames, ordered by frame, cube (raster), lane; scratch: slots
// [frames*cubes][8][4], counts [frames*cubes], sums [ceil(frames*cubes/1024)]; totals[0] = written, [1] = dropped.
// frame_count (nullable) selects the per-frame form: extrema is [frames][max_out][4], frame f's first max_out extrema at
// rows f * max_out .., frame_count[f] = all the frame holds; frame_of and totals are not written then
void launch_detect_extrema(const float *layer0, long layer0_stride, int layer0_pitch, const float *coarse, long coarse_stride,
                           long layer_stride, int n_layers, int w, int h, int frames, int border, int skip_layers,
                           float contrast_threshold, float *slots, unsigned *counts, unsigned *sums, float *extrema,
                           unsigned *frame_of, unsigned *frame_count, unsigned long long max_out,
                           unsigned long long *totals, hipStream_t stream, const RowBands *bands = nullptr);
// per frame: blobs with size >= min_size, the n_keep best by contrast, index order; out [n_frames][n_keep][4]
// (one list -- seg_count null: its length is read from n_in on the device, or taken from n_host when n_in is null;
// n_frames lists -- seg_count[f] extrema of frame f, the first min(., seg_cap) of them stored from row f * seg_cap)
void launch_topk_filter(const float *extrema, const unsigned *seg_count, const unsigned long long *n_in,
                        unsigned long long n_host, unsigned n_frames, unsigned seg_cap, unsigned n_keep, float min_size,
                        float *out, unsigned *out_index, unsigned *out_count, unsigned long long *out_count64,
                        unsigned long long n_cap, unsigned *work, hipStream_t stream);
// u32 words of `work` for lists of up to n_cap extrema (work may be null: one workgroup per frame is used then)
size_t topk_work_words(unsigned long long n_cap);
// per-frame padded selections [frames][n_keep] + counts -> contiguous list + frame ids; totals[0] = entries,
// totals[1] = extrema dropped by the per-frame cap seg_cap (seg_count[f]: extrema frame f holds)
void launch_segments_compact(const float *padded, const unsigned *counts, const unsigned *seg_count, unsigned n_frames,
                             unsigned seg_cap, unsigned n_keep, unsigned *offsets, float *out, unsigned *frame_of,
                             unsigned long long *totals, hipStream_t stream);

// brute-force matcher (csrc/mkd_match.hip): x [n][128] f32 -> f16 hi/lo operand tiles (match_tiles_bytes(n) bytes);
// a tiles against b tiles -> match [na] (index into b or -1) and optionally the best / second-best similarity.
// p_* hold splits x na partial results; excl_lo/hi (nullable): b rows [lo[i], hi[i]) are skipped for a row i.
size_t match_tiles_bytes(long n);
int match_splits(long na, long nb, int num_cus);
// norms [n] (nullable): |x_row| rounded up; max_norm_bits (nullable): running maximum of them as float bits
void launch_match_split(const float *x, long n, unsigned char *tiles, float *norms, unsigned *max_norm_bits,
                        hipStream_t stream);
// the three-term scan; n_over (nullable, device): as the fallback of the two-pass form the launch does nothing unless
// more rows overflowed than launch_match_few takes
void launch_match(const unsigned char *a_tiles, long na, const unsigned char *b_tiles, long nb, const unsigned *excl_lo,
                  const unsigned *excl_hi, float ratio, int splits, float *p_best, int *p_index, float *p_second,
                  int *match, float *best, float *second, const int *n_over, hipStream_t stream);
// small problems (match_small_fits: na * nb <= 2^23, nb <= 4096) in ONE launch straight from the f32 rows, no scratch; the
// three terms of the scan in its order.  overflowed_word (nullable): zeroed by the launch (this form redoes no row)
bool match_small_fits(long na, long nb);
void launch_match_small(const float *a, long na, const float *b, long nb, const unsigned *excl_lo, const unsigned *excl_hi,
                        float ratio, int *match, float *best, float *second, unsigned *overflowed_word, hipStream_t stream);
// both directions (a's rows against b, b's rows against a) in one launch; both must fit match_small_fits
void launch_match_small_both(const float *a, long na, const float *b, long nb, float ratio, int *match_ab, int *match_ba,
                             unsigned *overflowed_word, hipStream_t stream);
// n_pairs problems in one launch (lf_mkd_match_pairs_device): pair p = a rows [off_a[p], off_a[p+1]) against b rows
// [off_b[p], off_b[p+1]), offsets on the device and never read by the host; each pair decided by match_small's body.
// match_ba (nullable): the other direction from the same launch; mutual: two more element-wise launches keep only the
// matches both directions agree on.  match_pairs_slots: workgroups one direction over n_total rows takes.
uint64_t match_pairs_slots(uint64_t n_total, unsigned n_pairs);
void launch_match_small_pairs(const float *a, const uint64_t *off_a, uint64_t na_total, const float *b, const uint64_t *off_b,
                              uint64_t nb_total, unsigned n_pairs, float ratio, bool mutual, int *match_ab, int *match_ba,
                              float *best, float *second, unsigned *overflowed_word, hipStream_t stream);
// LF_MKD_MATCH_MUTUAL's two element-wise launches over both match arrays of such a batch (the guided call's as well)
void launch_match_mutual(const uint64_t *off_a, uint64_t na_total, const uint64_t *off_b, uint64_t nb_total, unsigned n_pairs,
                         int *match_ab, int *match_ba, hipStream_t stream);
// guided matching (csrc/mkd_match_guided.hip, lf_mkd_match_guided_pairs_device): the same batch, the same slot map and
// workgroup body, but a row's candidates are the rows of the other side that pass the verifier's inlier test with it under
// the pair's model [n_pairs][9] (kind 0: homography, 1: fundamental matrix); kps_a / kps_b rows of 5 floats (x, y read)
void launch_match_guided_pairs(const float *a, const float *kps_a, const uint64_t *off_a, uint64_t na_total, const float *b,
                               const float *kps_b, const uint64_t *off_b, uint64_t nb_total, const float *model,
                               unsigned n_pairs, unsigned kind, float threshold, float ratio, bool mutual, int *match_ab,
                               int *match_ba, float *best, float *second, hipStream_t stream);
// the same scan over the overflowed rows alone (few_words: their indices first, written by launch_match_verify)
size_t match_few_tiles_bytes();
size_t match_few_words();
void launch_match_few(const float *a, const unsigned char *b_tiles, long nb, const unsigned *excl_lo,
                      const unsigned *excl_hi, float ratio, const int *n_over, unsigned char *few_tiles, unsigned *few_words,
                      int *match, float *best, float *second, hipStream_t stream);
// the two-pass form: screen (one-term scan, candidate records per a row) then verify (exact f32 re-scoring, decision);
// *n_over (device, zeroed by the caller) counts a rows whose records overflowed
size_t match_record_bytes(long na, int splits);
size_t match_count_bytes(long na, int splits);
// shared_floor [na] ints (nullable): scratch through which the b splits of a query tell each other their running bounds
void launch_match_screen(const unsigned char *a_tiles, long na, const unsigned char *b_tiles, long nb,
                         const unsigned *excl_lo, const unsigned *excl_hi, int splits, const float *a_norms,
                         const unsigned *b_max_norm_bits, void *rec, void *rec_info, hipStream_t stream,
                         int *shared_floor = nullptr);
void launch_match_verify(const float *a, long na, const float *b, const float *a_norms, const unsigned *b_max_norm_bits,
                         const void *rec, const void *rec_info, int splits, float ratio, int *match, float *best,
                         float *second, int *n_over, int *over_rows, hipStream_t stream);

// 8-bit descriptors (csrc/mkd_match_q8.hip; include/lf_mkd.h): x [n][128] f32 -> q [n][128] offset-binary bytes,
// byte = clamp(rint(x * scale), -127, 127) + 128 (NaN -> 128)
void launch_quantize_rows(const float *x, unsigned long long n, float scale, unsigned char *q, hipStream_t stream);
// the exact int8 matcher's grid and scratch for a problem size: what lf_mkd_match_q8_plan reports and launch_match_q8 launches
struct Q8Plan {
    unsigned a_blocks, splits;         // the scan's grid; splits == 1: it writes the result itself, no merge launch
    long tiles_per_split;              // 32-row b tiles one split scans
    unsigned long long scratch_bytes;  // partial (best, second, index) per (split, a row); 0 exactly when splits == 1
};
Q8Plan match_q8_plan(long na, long nb, int num_cus);
// a [na][128] against b [nb][128] bytes -> match [na], best / second (nullable) as exact int32 sums; scratch: plan.scratch_bytes
void launch_match_q8(const unsigned char *a, long na, const unsigned char *b, long nb, const unsigned *excl_lo,
                     const unsigned *excl_hi, float ratio, const Q8Plan &plan, void *scratch, int *match, int *best,
                     int *second, hipStream_t stream);
// the exact top-k over 8-bit rows (csrc/mkd_match_q8_knn.hip, lf_mkd_knn_q8_device): what lf_mkd_knn_q8_plan reports and
// launch_knn_q8 launches
struct KnnQ8Plan {
    unsigned a_blocks, splits;         // the scan's grid; splits == 1: it writes the result itself, no merge launch
    long tiles_per_split;              // 32-row b tiles one split scans
    unsigned long long scratch_bytes;  // k 64-bit keys per (split, a row); 0 exactly when splits == 1
};
KnnQ8Plan knn_q8_plan(long na, long nb, int k, int num_cus);
unsigned knn_q8_block_rows();
// a [na][128] against b [nb][128] bytes -> index / score (nullable) [na][k], 1 <= k <= LF_MKD_KNN_MAX: each row's k best
// candidates, larger sum first, among equal sums the higher index first; scratch: plan.scratch_bytes
void launch_knn_q8(const unsigned char *a, long na, const unsigned char *b, long nb, const unsigned *excl_lo,
                   const unsigned *excl_hi, int k, const KnnQ8Plan &plan, void *scratch, int *index, int *score,
                   hipStream_t stream);
// grouped matching over 8-bit rows (csrc/mkd_match_q8_grouped.hip, lf_mkd_match_q8_grouped_device): what
// lf_mkd_match_q8_grouped_plan reports and launch_match_q8_grouped launches
struct Q8GroupedPlan {
    unsigned a_blocks, splits;         // the scan's grid; splits == 1: it writes the result itself, no merge launch
    long tiles_per_split;              // 32-row b tiles one split scans
    unsigned long long scratch_bytes;  // one 16-byte state per (split, a row); 0 exactly when splits == 1
};
Q8GroupedPlan match_q8_grouped_plan(long na, long nb, int num_cus);
unsigned match_q8_grouped_block_rows();
// a [na][128] against b [nb][128] bytes with group_of_b [nb] -> match [na], best / rival (nullable) [na]: the best candidate
// and the best score among the candidates of another group than the best's; scratch: plan.scratch_bytes
void launch_match_q8_grouped(const unsigned char *a, long na, const unsigned char *b, long nb, const unsigned *group_of_b,
                             const unsigned *excl_lo, const unsigned *excl_hi, float ratio, const Q8GroupedPlan &plan,
                             void *scratch, int *match, int *best, int *rival, hipStream_t stream);
// votes [n_groups_a][n_groups_b] = 0, then += 1 per row with 0 <= match < nb and both group ids in range (two launches);
// group_of_a nullable: group 0
void launch_vote_groups(const int *match, long na, const unsigned *group_of_a, unsigned n_groups_a,
                        const unsigned *group_of_b, long nb, unsigned n_groups_b, unsigned *votes, hipStream_t stream);
// many pairs of 8-bit rows in one launch (lf_mkd_match_q8_pairs_device): launch_match_small_pairs' layout and slot map at
// match_q8_pairs_block_rows() rows per workgroup; each pair decided as launch_match_q8 decides it alone.  No scratch.
// match_ba (nullable): the other direction from the same launch; mutual: launch_match_mutual's two launches on top.
unsigned match_q8_pairs_block_rows();
uint64_t match_q8_pairs_slots(uint64_t n_total, unsigned n_pairs);
void launch_match_q8_pairs(const unsigned char *a, const uint64_t *off_a, uint64_t na_total, const unsigned char *b,
                           const uint64_t *off_b, uint64_t nb_total, unsigned n_pairs, float ratio, bool mutual, int *match_ab,
                           int *match_ba, int *best, int *second, hipStream_t stream);
// edge-list matching over 8-bit rows (csrc/mkd_match_q8_edges.hip; include/lf_mkd.h, "edge lists").  A pool is a row array and
// image_off [n_images + 1]; an edge is two image ids; the edge layout of a side is a pair layout whose pair e has the rows of
// that side's image of edge e.
// edge_off [n_edges + 1] = the exclusive prefix sum of the edges' image row counts (two launches, one up to 1024 edges)
void launch_edge_layout(const uint64_t *image_off, unsigned n_images, uint64_t total, const unsigned *edge_image,
                        unsigned n_edges, uint64_t *edge_off, hipStream_t stream);
// rows of row_bytes bytes (a multiple of 4) from the pool into the edge layout; one launch over
// capacity / gather_edge_rows_block_rows() + n_edges workgroups
unsigned gather_edge_rows_block_rows();
void launch_gather_edge_rows(const void *src, unsigned row_bytes, const uint64_t *image_off, unsigned n_images, uint64_t total,
                             const unsigned *edge_image, const uint64_t *edge_off, uint64_t capacity, unsigned n_edges, void *dst,
                             hipStream_t stream);
// every edge decided as launch_match_q8 decides its two images alone, outputs in the edge layouts; launch_match_q8_pairs' grid
// over (ea_capacity, eb_capacity, n_edges).  edge_off_b / match_ba nullable together; mutual: launch_match_mutual on top.
void launch_match_q8_edges(const unsigned char *a, const uint64_t *image_off_a, unsigned n_images_a, uint64_t na_total,
                           const unsigned char *b, const uint64_t *image_off_b, unsigned n_images_b, uint64_t nb_total,
                           const unsigned *edge_a, const unsigned *edge_b, const uint64_t *edge_off_a, uint64_t ea_capacity,
                           const uint64_t *edge_off_b, uint64_t eb_capacity, unsigned n_edges, float ratio, bool mutual,
                           int *match_ab, int *match_ba, int *best, int *second, hipStream_t stream);
// feature tracks (csrc/mkd_tracks.hip, lf_mkd_build_tracks_device): track [total] = the smallest row of every row's connected
// component under the links match (in edge_off's layout, against capacity) holds; accumulate: track is the forest an earlier
// call left and is not initialised.  len / dup (nullable) [total]: per label the rows of the track and its conflicting rows.
// Launches: init (not under accumulate), link over capacity / build_tracks_link_entries() + n_edges workgroups (only with
// n_edges > 0), flatten; with a statistic: zero, len (if given), dup over total / build_tracks_dup_tile() + n_images
// workgroups (if given and n_images > 0).  total == 0: nothing.  No scratch.
unsigned build_tracks_link_entries();
unsigned build_tracks_dup_tile();
void launch_build_tracks(const uint64_t *image_off, unsigned n_images, uint64_t total, const unsigned *edge_a,
                         const unsigned *edge_b, const uint64_t *edge_off, uint64_t capacity, unsigned n_edges, const int *match,
                         bool accumulate, int *track, unsigned *len, unsigned *dup, hipStream_t stream);
// track tables (csrc/mkd_track_table.hip, lf_mkd_track_table_device / lf_mkd_gather_track_rows_device).  The plan is the one
// place that knows the digit width and the block size: key_bits = the bits of floor(total / min_len), passes radix passes of
// blocks of block_rows rows, and the layout of the scratch (byte offsets; blk_len sits at 0).  key_none: the key of a row of no
// kept track, above every table index.
// Launches: total == 0: one (zeroes).  Otherwise select, scan_blocks, apply, keys; then, unless passes == 0 or obs_capacity
// == 0, three per pass (hist, scan_hist, scatter) and finalise.  gather: one, over ceil(obs_capacity / 64) workgroups.
struct TrackTablePlan {
    unsigned key_bits, passes, block_rows, key_none;
    uint64_t n_blocks, off_map, off_keys[2], off_rows[2], off_blk_cnt, off_hist, off_totals, scratch_bytes;
};
TrackTablePlan track_table_plan(uint64_t total, unsigned min_len);
void launch_track_table(const TrackTablePlan &plan, unsigned char *scratch, const uint64_t *image_off, unsigned n_images,
                        uint64_t total, const int *track, const unsigned *len, const unsigned *dup, unsigned min_len,
                        uint64_t track_capacity, uint64_t obs_capacity, uint64_t *offsets, int *obs_row, unsigned *obs_image,
                        int *row_track, unsigned *counts, hipStream_t stream);
void launch_gather_track_rows(const void *src, unsigned row_bytes, uint64_t total, const int *obs_row, const unsigned *counts,
                              uint64_t obs_capacity, void *dst, hipStream_t stream);
// link tables (csrc/mkd_link_table.hip, lf_mkd_link_table_device).  The plan is the one place that knows the slot size and the
// scan's fan-out: slots = floor(capacity / slot_entries) + n_edges (tracks_link's grid), scan_levels = the smallest L with
// scan_fanout^L >= slots (0 for n_edges == 0), level k = 1 .. L - 1 of the scan has level_n[k] values, and the layout of the
// scratch (byte offsets; the slots' W sits at 0).
// Launches: n_edges == 0: one (zeroes).  Otherwise zero, count, L - 1 up, L down, cut, scatter (not when link_capacity == 0
// and match_kept is null), finalise: 2 L + 4 or 2 L + 3.
struct LinkTablePlan {
    unsigned slot_entries, scan_fanout, scan_levels;
    uint64_t slots, level_n[8], off_level_links[8], off_level_edges[8], off_totals, off_slot_cnt, off_slot_edge, off_slot_idx,
        off_edge_links, scratch_bytes;
};
LinkTablePlan link_table_plan(uint64_t capacity, unsigned n_edges);
void launch_link_table(const LinkTablePlan &plan, unsigned char *scratch, const uint64_t *image_off, unsigned n_images,
                       uint64_t total, const unsigned *edge_a, const unsigned *edge_b, const uint64_t *edge_off, uint64_t capacity,
                       unsigned n_edges, const int *match, unsigned min_links, bool local, uint64_t link_capacity,
                       uint64_t *offsets, int *link_a, int *link_b, unsigned *link_edge, unsigned *edge_links, int *match_kept,
                       unsigned *counts, hipStream_t stream);
// candidate edges (csrc/mkd_select_edges.hip, lf_mkd_select_edges_device).  The plan is the one place that knows the forms:
// compiled_k = the instantiation that serves k (4, 8, 16, 32); rows_per_workgroup = 4 (one wave per row: rows of at most 2048
// columns) or 1; splits = the segments of `segment` columns a row is cut into (1 unless there are fewer than 1024 rows of more
// than 4096 columns); workgroups = the selection's grid; slots = n_a k, blocks = ceil(slots / 256) (the grid of the flags);
// the layout of the scratch (byte offsets; the segments' keys sit at 0).
// Launches: n_a == 0: one (counts and padding).  Otherwise select, merge (splits > 1 only), flag, scan, scatter: 4 or 5.
struct SelectEdgesPlan {
    unsigned compiled_k, rows_per_workgroup, splits, segment, launches;
    uint64_t workgroups, slots, blocks, off_rank, off_rank_votes, off_local, off_blocks, scratch_bytes;
};
SelectEdgesPlan select_edges_plan(unsigned n_a, unsigned n_b, unsigned k, uint64_t edge_capacity);
void launch_select_edges(const SelectEdgesPlan &plan, unsigned char *scratch, const unsigned *votes, unsigned n_a, unsigned n_b,
                         unsigned k, unsigned min_votes, bool skip_self, bool unique, uint64_t edge_capacity, int *rank,
                         unsigned *rank_votes, unsigned *edge_a, unsigned *edge_b, unsigned *edge_votes, unsigned *counts,
                         hipStream_t stream);
// covisibility tables (csrc/mkd_covisibility.hip, lf_mkd_covisibility_device).  The plan is the one place that knows the forms:
// group = the lanes that share a track in cv_short (4 .. 64: the smallest power of two that holds twice the mean track length
// the capacities allow, never more than the images there are); lds = 1 iff a workgroup counts into a private table in LDS
// first (n_images <= LF_COVIS_LDS_IMAGES = 64; its grid is then held to 2^22 / n_images^2 workgroups, at least 256); the grids; bitmap_words = the scratch: one bit per 64 positions of the observation
// array, set for the chunks of the tracks cv_short leaves to cv_long (more than 16 * group positions).
// Launches: n_images == 0: none.  Otherwise zero, short and long (not with a capacity of 0), mask (n_edges > 0 only).
struct CovisibilityPlan {
    unsigned group, lds, zero_blocks, short_blocks, long_blocks, mask_blocks, launches;
    uint64_t bitmap_words, scratch_bytes;
};
CovisibilityPlan covisibility_plan(unsigned n_images, uint64_t track_capacity, uint64_t obs_capacity, uint64_t n_edges);
void launch_covisibility(const CovisibilityPlan &plan, unsigned char *scratch, const uint64_t *track_offsets,
                         uint64_t track_capacity, const unsigned *obs_image, uint64_t obs_capacity, const unsigned *table_counts,
                         unsigned n_images, const unsigned *edge_a, const unsigned *edge_b, uint64_t n_edges, bool accumulate,
                         unsigned *covis, hipStream_t stream);
// two-view poses (csrc/mkd_two_view_pose.hip, lf_mkd_two_view_pose_device): one launch, a workgroup per edge, no scratch.
// Keypoints are read as rows of 5 floats; cmin = the cosine of the parallax threshold, formed by the host in double.
void launch_two_view_pose(const float *kps, uint64_t n_rows, const unsigned *edge_a, const unsigned *edge_b, unsigned n_edges,
                          const float *intrinsics, unsigned n_images, const float *F, const uint64_t *link_off, const int *link_a,
                          const int *link_b, uint64_t link_capacity, double cmin, float *R, float *t, unsigned *stats, float *sigma,
                          float *points, hipStream_t stream);
// The reconstruction stages below take a scene's tables -- keypoints, image and track offsets, observations, capacities,
// counts, row_track, intrinsics -- as ONE SceneTables (mkd_scene.h), filled by the entry point after its refusals; a member a
// stage does not read is null or 0 (triangulation: off, row_track; resection: toff, obs_row, obs_image, ocap; bundle
// adjustment: row_track).  Points, poses and thresholds stay arguments of their own.
// track triangulation (csrc/mkd_triangulate.hip, lf_mkd_triangulate_tracks_device): one launch, 4 lanes per track, no scratch.
// Keypoints are read as rows of 5 floats; thr2 = the squared reprojection threshold, formed by the host in double.
void launch_triangulate_tracks(const SceneTables &tables, const float *poses, double thr2, unsigned rounds, float *points,
                               unsigned *stats, float *err, unsigned *obs_state, hipStream_t stream);
// track descriptors (csrc/mkd_track_desc.hip, lf_mkd_track_descriptors_device): one launch, 8 lanes per track, no scratch.
// The tables read are toff, tcap, obs_row, ocap, counts and n_rows (the rows of q); cmin = the cosine of the smallest
// parallax, formed by the host in double; scale > 0.  obs_state, points and stats may be null.
void launch_track_descriptors(const SceneTables &tables, const unsigned char *q, const unsigned *obs_state, unsigned min_state,
                              const float *points, double cmin, float scale, unsigned char *desc, int *stats, hipStream_t stream);
// camera resection (csrc/mkd_resect.hip, lf_mkd_resect_cameras_device): three launches (rs_gather, rs_score, rs_select) over
// `scratch` of resect_scratch_bytes(..) bytes, 4-byte aligned.  thr2 = the squared reprojection threshold and cmin = the
// cosine of the smallest parallax, both formed by the host in double.  poses_out may be poses.
uint64_t resect_scratch_bytes(unsigned n_images, uint64_t n_rows, unsigned n_samples);
void launch_resect_cameras(void *scratch, const SceneTables &tables, const float *points, const float *poses, double thr2,
                           double cmin, unsigned n_samples, unsigned min_inliers, unsigned rounds, unsigned seed, bool all,
                           float *poses_out, unsigned *stats, float *err, unsigned *row_state, hipStream_t stream);
// bundle adjustment (csrc/mkd_bundle.hip, lf_mkd_bundle_adjust_device): bundle_launches(..) launches over `scratch` of
// bundle_scratch_bytes(..) bytes, 16-byte aligned.  thr2 = the squared reprojection threshold and tol2 = the squared CG
// tolerance, both formed by the host in double.  poses_out may be poses, points_out points, obs_state_out obs_state.
uint64_t bundle_scratch_bytes(unsigned n_images, uint64_t n_rows, uint64_t track_capacity, uint64_t obs_capacity);
unsigned bundle_launches(unsigned iterations, unsigned cg_iterations);
void launch_bundle_adjust(void *scratch, const SceneTables &tables, const float *points, const float *poses,
                          const unsigned *obs_state, const unsigned *camera_fixed, double thr2, double lambda0, unsigned iterations,
                          unsigned cg_iterations, double tol2, float *poses_out, float *points_out, unsigned *obs_state_out,
                          double *trace, unsigned *counts, hipStream_t stream);
// the same with shared intrinsics refined (lf_mkd_bundle_adjust_intrinsics_device): the same kernels in their double-K form
// and three per-group ones, bundle_intrinsics_launches(..) launches over bundle_intrinsics_scratch_bytes(..) bytes.
// camera_group and group_out may be null; intrinsics_out may be intrinsics.
uint64_t bundle_intrinsics_scratch_bytes(unsigned n_images, uint64_t n_rows, uint64_t track_capacity, uint64_t obs_capacity,
                                         unsigned n_groups);
unsigned bundle_intrinsics_launches(unsigned iterations, unsigned cg_iterations);
void launch_bundle_adjust_intrinsics(void *scratch, const SceneTables &tables, const float *points, const float *poses,
                                     const unsigned *obs_state, const unsigned *camera_fixed, const unsigned *camera_group,
                                     unsigned n_groups, unsigned refine, double thr2, double lambda0, unsigned iterations,
                                     unsigned cg_iterations, double tol2, float *poses_out, float *points_out, float *intrinsics_out,
                                     float *group_out, unsigned *obs_state_out, double *trace, unsigned *counts, hipStream_t stream);
// view-graph checks (csrc/mkd_view_graph.hip, lf_mkd_view_graph_device).  The plan is the one place that knows the launches and
// the layout of the scratch (byte offsets, 8-byte aligned): the edges' quaternions f64 [n_edges][4], the images' quaternions
// f64 [2][n_images][4] (the sweeps go from one to the other), then the pair table uint32 [n_images][n_images].
// Launches: n_images == 0: none.  Otherwise zero, edges and vote (n_edges > 0 only), root, tree_rounds, iterations, final,
// filter (a match array and n_edges > 0 only): 3 + tree_rounds + iterations, + 2 or 3 with edges.
// cmax = the cosine of the loop threshold, formed by the host in double.  match_out may be match.  Returns the launches it
// issued, which the entry point holds against the plan's.
struct ViewGraphPlan {
    unsigned launches;
    uint64_t off_edge_quat, off_quat[2], off_table, scratch_bytes;
};
ViewGraphPlan view_graph_plan(unsigned n_images, unsigned n_edges, unsigned tree_rounds, unsigned iterations, bool filter);
unsigned launch_view_graph(const ViewGraphPlan &plan, unsigned char *scratch, const unsigned *edge_a, const unsigned *edge_b,
                       unsigned n_edges, const float *R, const unsigned *pose_stats, unsigned n_images, double cmax,
                       unsigned min_front, unsigned root, unsigned tree_rounds, unsigned iterations, bool use_unchecked,
                       const uint64_t *edge_off, uint64_t capacity, const int *match, int *match_out, float *rotations,
                       unsigned *edge_stats, float *residual, unsigned *image_stats, unsigned *counts, hipStream_t stream);
// tree poses (csrc/mkd_positions.hip, lf_mkd_tree_poses_device): one launch, a thread per image, no scratch.
void launch_tree_poses(const unsigned *edge_a, const unsigned *edge_b, const float *t, unsigned n_edges, const float *rotations,
                       const unsigned *image_stats, unsigned n_images, unsigned max_depth, float *poses, hipStream_t stream);
// global positions (csrc/mkd_positions.hip, lf_mkd_global_positions_device).  The plan is the one place that knows the launches
// (4 + 3 sweeps: init, gauge, then points, cameras and gauge per sweep, final images, final tracks; none for n_images == 0)
// and the layout of the scratch (byte offsets, 16-byte aligned): the centres f64 [n_images][3], the points f64
// [track_capacity][3], the rotations f32 [n_images][9], registered, held and reason uint32 [n_images] each, the points' flags
// uint32 [track_capacity], four words, the latest gauge f64 [4].  s0 = the sine of the robust angle, formed by the host in double.  poses_out may be
// poses.  Returns the launches it issued, which the entry point holds against the plan's.
struct GlobalPositionsPlan {
    unsigned launches;
    uint64_t off_cen, off_pt, off_rot, off_reg, off_held, off_reason, off_tflag, off_words, off_gauge, scratch_bytes;
};
GlobalPositionsPlan global_positions_plan(unsigned n_images, uint64_t track_capacity, unsigned sweeps);
unsigned launch_global_positions(const GlobalPositionsPlan &plan, unsigned char *scratch, const SceneTables &tables,
                                 const float *poses, unsigned sweeps, unsigned warm, double s0, unsigned min_obs, float *poses_out,
                                 float *points_out, unsigned *obs_state, unsigned *image_stats, double *trace, unsigned *counts,
                                 hipStream_t stream);
// guided matching over 8-bit rows (csrc/mkd_match_q8_guided.hip, lf_mkd_match_q8_guided_pairs_device): launch_match_q8_pairs'
// batch, grid and sums, launch_match_guided_pairs' candidates (the same keypoints, model, kind and threshold)
void launch_match_q8_guided_pairs(const unsigned char *a, const float *kps_a, const uint64_t *off_a, uint64_t na_total,
                                  const unsigned char *b, const float *kps_b, const uint64_t *off_b, uint64_t nb_total,
                                  const float *model, unsigned n_pairs, unsigned kind, float threshold, float ratio, bool mutual,
                                  int *match_ab, int *match_ba, int *best, int *second, hipStream_t stream);

// RANSAC homography verification (mkd_verify.hip; algorithm: include/lf_mkd.h).  Keypoints are read as rows of 5 floats
// (lf_mkd_keypoint).  Scratch the caller owns: pairs [n_pairs], counts [n_pairs][slices][n_hyp]; `verified` also holds each
// pair's list of considered rows between the first and the last of the call's three launches.
// (VerifyPair, a pair's normalisation: mkd_verify_pair.h)
// row slices per (pair, hypothesis block) of the scoring launch: enough workgroups to fill the chip for few pairs
unsigned verify_slices(unsigned n_pairs, unsigned n_hyp, int num_cus);
void launch_verify(const float *kps_a, const uint64_t *off_a, const float *kps_b, const uint64_t *off_b, const int *match,
                   unsigned n_pairs, unsigned n_hyp, float threshold, unsigned seed, unsigned flags, unsigned slices,
                   VerifyPair *pairs, unsigned *counts, float *H, int *verified, unsigned *stats, hipStream_t stream);
// launch 1 of both verifiers alone (include/lf_mkd.h, step 1): each pair's considered rows by ascending row into `list`
// (indexed like match), and its normalisation into pairs[p]
void launch_verify_prepare(const float *kps_a, const uint64_t *off_a, const float *kps_b, const uint64_t *off_b, const int *match,
                           unsigned n_pairs, VerifyPair *pairs, int *list, hipStream_t stream);
// RANSAC fundamental matrix (mkd_verify.hip as well; algorithm: include/lf_mkd.h).  Scratch: pairs [n_pairs], counts
// [n_pairs][slices][n_hyp][3] (one count per candidate of a sample; slices from verify_slices, the same grid shape);
// `verified` holds the considered rows as above.
void launch_fundamental(const float *kps_a, const uint64_t *off_a, const float *kps_b, const uint64_t *off_b, const int *match,
                        unsigned n_pairs, unsigned n_hyp, float threshold, unsigned seed, unsigned flags, unsigned slices,
                        VerifyPair *pairs, unsigned *counts, float *F, int *verified, unsigned *stats, hipStream_t stream);

#ifdef __HIPCC__
// Which tile a workgroup takes, for the row-tiled pyramid and a-trous kernels: workgroups are dealt to the 8 XCDs round-robin by their
// linear id, so the tiles above and below a tile -- which read the same halo rows -- would sit on other XCDs, behind other
// L2s, and every halo row would come from HBM once per tile.  The remap (bijective for any workgroup count) hands each
// group of workgroups that share an XCD a contiguous run of tiles in (x fastest, then y, then frame) order.  (Measured on the
// staged kernels of mkd_pyramid.hip: the frame is then read from HBM once, 0.315 instead of 0.459 GB per 256 frames, and
// the launch is ~5 % shorter; the extremum scan and the decimating kernel did not gain and keep blockIdx.)
struct TileId { unsigned x, y, z; };
__device__ __forceinline__ TileId xcd_tile() {
    const unsigned nwg = gridDim.x * gridDim.y * gridDim.z;
    const unsigned id = blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z);
    const unsigned xcd = id % 8u, q = nwg / 8u, r = nwg % 8u;
    const unsigned t = (xcd < r ? xcd * (q + 1u) : r * (q + 1u) + (xcd - r) * q) + id / 8u;
    const unsigned row = t / gridDim.x;
    return TileId{t - row * gridDim.x, row % gridDim.y, row / gridDim.y};
}

#endif

}  // namespace lfmkd
