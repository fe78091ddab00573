/*
 * lf_mkd.h -- C ABI of the MI355X-native MKD descriptor path (liblf_mkd.so).
 *
 * This is the drop-in boundary for ONE path of tnibler/local-features: the
 * "describe" half of LocalFeaturesVulkan::detect (local_features/src/vulkan/mod.rs:435-453),
 * i.e. the extract task graph (mod.rs:1277-1572):
 *   keypoint orientation -> patch sampling -> blur/gradients -> von-Mises x spatial-kernel
 *   pooling -> normalise -> PCA whitening -> L2.
 * Plain pointers and sizes only; no C++/torch types.  Each entry point cites the
 * reference interface it replaces.  The Rust-side binding a maintainer would add
 * is shown in INTEGRATION.md.
 *
 * Threading: a handle is NOT thread-safe (the reference takes &mut self on every
 * call, mod.rs:346-367); use one handle per device/stream.  Different handles may be
 * used from different host threads at the same time (one thread per handle).  All functions return
 * LF_MKD_OK (0) or a negative lf_mkd_status; they never abort.  The message for
 * the last failure on a handle is available from lf_mkd_last_error().
 *
 * Current device: every entry point makes the handle's device (lf_mkd_params.device) current
 * for its own duration and puts the calling thread's current HIP device back before it returns,
 * on every return path -- a process that drives one handle per GPU keeps the current device it
 * had (one hipGetDevice per call; hipSetDevice only when the two differ).
 */
#ifndef LF_MKD_H
#define LF_MKD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LF_MKD_PATCH_SIZE 32       /* lib.rs:15  PATCH_SIZE            */
#define LF_MKD_RAW_LEN 238         /* lib.rs:12  RAW_DESCRIPTOR_LEN    */
#define LF_MKD_DESC_LEN 128        /* lib.rs:13  DESCRIPTOR_LEN        */

typedef enum {
    LF_MKD_OK = 0,
    LF_MKD_ERR_BAD_ARG = -1,   /* null pointer, zero size, image larger than max_image_* ... */
    LF_MKD_ERR_HIP = -2,       /* a HIP runtime call failed; see lf_mkd_last_error         */
    LF_MKD_ERR_IO = -3,        /* cannot read / parse the PCA model file                   */
    LF_MKD_ERR_NO_IMAGE = -4,  /* describe_keypoints before set_image                      */
    LF_MKD_ERR_NO_DEVICE = -5, /* no usable gfx950 device                                  */
    LF_MKD_ERR_COMM = -6       /* RCCL is not loadable, or one of its calls failed         */
} lf_mkd_status;

/* Which PCA model to load from a model directory: enum MKDPCA, lib.rs:26-32. */
typedef enum { LF_MKD_PCA_LIBERTY = 0, LF_MKD_PCA_NOTREDAME = 1, LF_MKD_PCA_YOSEMITE = 2 } lf_mkd_pca;

/* Angle path of the gradient stage.
 * SHADER  : the reference's polynomial atan2 incl. its quirks (shaders/atan2.glsl:19-46). Default.
 *           (Domain: gx == -0.0 is gx == 0, as in the shader.  A gradient whose LARGER component is below 1e-30 in
 *           magnitude -- pixel values of that order; frames of [0, 1] have none -- gets the direction of
 *           min / max(larger, 1e-30) instead of min / larger: the hardware reciprocal has no denormal range.)
 * EXACT   : cos/sin of the gradient direction taken as gx/|g|, gy/|g| (what the polynomial
 *           approximates to 1e-5 rad; matches mkd_ref.rs:140, the CPU twin).
 * EXACT_ZERO : EXACT, except that a pixel with gx == 0 gets angle 0 as in the shader.  That is the one input
 *           where SHADER and EXACT are far apart (0 against +-pi/2), so this mode stays within 1e-4 relative L2 of
 *           the shader reference on EVERY patch (measured <= 3e-5) at EXACT's cost (about 11 % cheaper than SHADER). */
typedef enum { LF_MKD_ANGLE_SHADER = 0, LF_MKD_ANGLE_EXACT = 1, LF_MKD_ANGLE_EXACT_ZERO = 2 } lf_mkd_angle_mode;

/* Arithmetic of the pooling contraction (1024 px x 7 in-dims x 34 kernels per patch).
 * F16X3   : operands split into f16 hi+lo, three f16 MFMAs per product (hi*hi, hi*lo, lo*hi),
 *           f32 accumulate; ~2^-21 relative per product -- descriptors within 1e-5 relative L2 of the f32
 *           formulation (gate 1e-4).  THE DEFAULT (a zero-initialised lf_mkd_params selects it): ~250 M
 *           descriptors/s per MI355X in patch mode.
 * F32     : v_mfma_f32_16x16x4_f32, bit-for-bit an f32 fma chain; the verification mode, bound by the f32 MFMA
 *           rate at ~117 M descriptors/s (2.1x slower).
 * F16_FP6 : an experiment kept as a mode (round 4, NOTEBOOK.md section 11): hi*hi in f16 as above, the two cross terms of the
 *           harmonics' streams in ONE block-scaled v_mfma_scale_f32_16x16x128_f8f6f4 per accumulator tile with e2m3
 *           operands (51 instead of the 81 matrix instructions per wave-row of the unfolded three-term form it was built on and
 *           keeps; the default has since folded its rows to 63 and is the faster of the two).  e2m3 carries three bits below its block's
 *           maximum: descriptors within 3e-5 of the oracle (measured worst 2.95e-5, mean 2.0e-5, over the goldens and 4099
 *           patches x 3 angle modes x both kernel forms; F16X3: 4.2e-6 / 3.1e-6 -- seven times the error, inside the gate; the
 *           -m gpu test holds it below 4e-5) for +2 % of speed over the unfolded F16X3 of its time -- NOT the default, not used for any reported parity figure.  Patch mode only: keypoint
 *           entry points take the two-launch form in this mode. */
typedef enum { LF_MKD_POOL_DEFAULT = 0, LF_MKD_POOL_F16X3 = 1, LF_MKD_POOL_F32 = 2, LF_MKD_POOL_F16_FP6 = 3 } lf_mkd_pool_mode;

/* lf_mkd_params.flags */
#define LF_MKD_FLAG_KERNEL_TIMING 1u /* bracket every kernel launch with HIP events on its stream;
                                        read the sums with lf_mkd_kernel_times (bench.py's roofline) */
#define LF_MKD_FLAG_UNFUSED_KEYPOINTS 2u /* keypoint mode as two launches: the sampler writes the 32x32 patches to a staging
                                        buffer in HBM, the patch kernel reads them back (the verification form: same bits).
                                        By default patches are sampled inside the describe kernel -- producer waves of each
                                        workgroup fill its LDS row ring, patch_gradients.glsl:42-70 -- and never touch HBM.
                                        (LF_MKD_POOL_F32 always takes the two-launch form.) */

#define LF_MKD_FLAG_DETECT_STEPWISE 4u /* lf_mkd_detect / lf_mkd_detect_u8 stage by stage, every count fetched by the host before the
                                        next stage is sized (three waits): the verification form.  By default every count stays
                                        on the device, and the whole pipeline is ONE hipGraph launch, recorded the second time a
                                        (frame size, top_n, min_size, max_out, pixel type) is asked for and kept; same bits. */

/* Mirrors BuildTimeParams (lib.rs:54-75) + FeatureDetectParams (lib.rs:34-52) for this path.
 * Zero-initialise, then set what you need; 0 means "default". */
typedef struct {
    uint32_t max_image_width;   /* BuildTimeParams.max_image_width  (0: keypoint mode unused) */
    uint32_t max_image_height;  /* BuildTimeParams.max_image_height                            */
    uint32_t max_features;      /* BuildTimeParams.max_features: descriptors per internal batch;
                                   larger requests are processed in batches (default 2000 -> raised
                                   to a multiple of 64) */
    float patch_scale_factor;   /* FeatureDetectParams.patch_scale_factor (default 24)         */
    int32_t device;             /* HIP device ordinal                                          */
    int32_t angle_mode;         /* lf_mkd_angle_mode                                           */
    int32_t pool_mode;          /* lf_mkd_pool_mode (0 = LF_MKD_POOL_F16X3)                    */
    uint32_t flags;             /* LF_MKD_FLAG_*                                               */
    uint32_t max_frames;        /* frames of max_image_* size the pyramid store holds for the
                                   multi-frame entry points (default 1)                         */
    uint32_t n_scales;          /* BuildTimeParams.n_scales (lib.rs:60, default 4): keypoint orientation
                                   reads an a-trous stack of n_scales + 3 layers                */
    uint32_t max_blobs;         /* BuildTimeParams.max_blobs (lib.rs:58, default 8000): extrema the detector keeps
                                   per frame, rounded up to a multiple of 256 (mod.rs:279-286)   */
    uint32_t reserved[1];
} lf_mkd_params;

/* Keypoint as the path consumes it: struct Keypoint, lib.rs:17-24 (angle in DEGREES,
 * keypoint_orientation.glsl:162-167; response is carried through, not used). */
typedef struct {
    float x, y, size, angle, response;
} lf_mkd_keypoint;

/* Refined scale-space extremum as keypoint orientation reads it: the {x, y, scale, contrast} floats of
 * ExtremumLocations (shaders/common.glsl:45-81) for one index of FilteredExtrema (common.glsl:83-89),
 * gathered into an array of structs.  size = the interpolated scale written by refine_extrema. */
typedef struct {
    float x, y, size, response;
} lf_mkd_extremum;

#define LF_MKD_MAX_ANGLES_PER_EXTREMUM 18 /* strict local maxima of a circular 36-bin histogram */

typedef struct lf_mkd lf_mkd; /* opaque; owns all device memory */

/* Replaces new_vulkan() + upload_constant_data() for this path (lib.rs:94-100,
 * mod.rs:1587-1713).  PCA tensors are the three arrays of the reference's safetensors
 * model (mkd_ref.rs:352-391): mean[238], eigvals[238], eigvecs[238*238] row-major. */
int lf_mkd_create(const lf_mkd_params *params, const float *mean, const float *eigvals,
                  const float *eigvecs, lf_mkd **out);

/* Same, reading concat-pca-*.safetensors (models/mkd/, embedded by mkd_ref.rs:26-31). */
int lf_mkd_create_from_file(const lf_mkd_params *params, const char *safetensors_path,
                            lf_mkd **out);

void lf_mkd_destroy(lf_mkd *h);

const char *lf_mkd_last_error(const lf_mkd *h);

/* Patch mode: the extract graph from patch_gradients' blur onwards
 * (tasks_extract.rs:72-333; CPU twin Mkd::patch, mkd_ref.rs:57-77).
 * patches: [n][32][32] f32 row-major, out: [n][128] f32.  Host pointers; synchronous. */
int lf_mkd_describe_patches(lf_mkd *h, const float *patches, uint64_t n, float *out);

/* Same with DEVICE pointers, enqueued on `stream` (a hipStream_t, or NULL for the handle's
 * own stream); asynchronous.  This is what a caller that already holds patches in HBM uses. */
int lf_mkd_describe_patches_device(lf_mkd *h, const float *d_patches, uint64_t n, float *d_out,
                                   void *stream);

/* Debug/verification tap: un-whitened 238-D descriptor (RawDescriptorBuffer, common.glsl:133-139).
 * Device pointers, asynchronous. */
int lf_mkd_raw_descriptors_device(lf_mkd *h, const float *d_patches, uint64_t n, float *d_raw,
                                  void *stream);

/* Keypoint mode, step 1: upload one frame (f32 in [0,1], row-major, contiguous; mod.rs:368)
 * and build the patch pyramid (patch_pyramid.rs:38-156 + blur.glsl + swt.glsl level 0).
 * width/height must not exceed max_image_*; the pyramid mirrors at the content edge. */
int lf_mkd_set_image(lf_mkd *h, const float *image, uint32_t width, uint32_t height);
int lf_mkd_set_image_device(lf_mkd *h, const float *d_image, uint32_t width, uint32_t height,
                            void *stream);

/* The same from the 8-bit luma the reference's callers start from (`image::open(..).grayscale()`, then `convert()` to f32 / 255:
 * examples/match_images/src/main.rs:44-60; `u8 as f32 / 255.`: examples/webcam/src/main.rs:136): 1 byte per pixel over PCIe
 * instead of 4.  A pixel v becomes (float)v / 255.0f with a correctly rounded division on the device, i.e. the f32 frame the
 * host conversion gives, bit for bit: every result equals that of lf_mkd_set_image on the converted frame.  Row-major,
 * contiguous, width bytes per row. */
int lf_mkd_set_image_u8(lf_mkd *h, const uint8_t *image, uint32_t width, uint32_t height);
/* Device-pointer form, n_frames frames of one size, width * height bytes apart (n_frames <= max_frames). */
int lf_mkd_set_images_u8_device(lf_mkd *h, const uint8_t *d_images, uint32_t n_frames, uint32_t width, uint32_t height,
                                void *stream);

/* Multi-frame form of step 1 (BASELINE configs[2], [3]: hundreds of small frames): n_frames frames of one
 * size, contiguous [n_frames][height][width] in device memory, all pyramids built by one set of launches.
 * n_frames <= max_frames. */
int lf_mkd_set_images_device(lf_mkd *h, const float *d_images, uint32_t n_frames, uint32_t width,
                             uint32_t height, void *stream);

/* Keypoint mode, step 2: sample + describe (patch_gradients.glsl:42-70 onwards).
 * out: [n][128].  Host pointers; synchronous.
 * Forms of the launch, chosen by the size of the request (the capacity max_out for lf_mkd_detect* and lf_mkd_stream_*):
 *   whole-patch   one wave walks the 32 rows of its 16 patches and sums them in one chain: any size; ~72 us of latency
 *                 however few the keypoints;
 *   row-split     at most 4096 keypoints (16 x the chip's CUs; the reference's own settings are top_n 2000 / max_features
 *                 3000): the rows of a batch of 32 patches are shared by 4 workgroups (up to 2048 keypoints) or 2, whose
 *                 partial sums are added in a fixed order -- 43 us at 2000 keypoints, 50 at 3000.
 * Within a form a descriptor's bits depend on its keypoint and its frame alone (whatever else is in the request, however
 * often it is computed).  Between forms the pooled sums round differently: descriptors agree to ~3e-6 relative L2 (worst
 * measured 6.5e-6 over 32 000 soak launches; the tests hold 1e-5), both within the same distance of the reference.  LF_MKD_KP_SPLIT=1 in the
 * environment keeps every request in the whole-patch form (2 / 4: that row-split form wherever it fits).  (In the row-split
 * form a workgroup waits for its partners' partial sums; the wait is bounded, and a partial sum that never arrived -- a fault,
 * never observed -- is counted: lf_mkd_describe_keypoints then returns LF_MKD_ERR_HIP.) */
int lf_mkd_describe_keypoints(lf_mkd *h, const lf_mkd_keypoint *kps, uint64_t n, float *out);
int lf_mkd_describe_keypoints_device(lf_mkd *h, const lf_mkd_keypoint *d_kps, uint64_t n,
                                     float *d_out, void *stream);

/* Multi-frame form of step 2: d_frame_of_kp[i] (device, may be NULL = all frame 0) names the frame of
 * keypoint i among those given to lf_mkd_set_images_device.  One sampling launch + one describe launch
 * per internal batch, whatever the number of frames. */
int lf_mkd_describe_keypoints_frames_device(lf_mkd *h, const lf_mkd_keypoint *d_kps,
                                            const uint32_t *d_frame_of_kp, uint64_t n, float *d_out,
                                            void *stream);

/* Keypoint orientation: the first node of the extract graph (keypoint_orientation.glsl:36-171,
 * dispatched from mod.rs:1277-1344), i.e. what turns the detector's extrema into the keypoints the
 * describe entry points take.  Needs lf_mkd_set_image*: the first call after it extends the frame's
 * sigma-0.6 level into the a-trous stack of n_scales + 3 full-resolution layers (swt.glsl, mod.rs:1093-1130).
 * Every histogram peak >= 0.8 max yields one keypoint {x, y, size, angle = 360 - 10 bin, response}.
 * Output ORDER is defined here (the reference appends with an atomic counter, in no particular order):
 * by extremum index, then by ascending histogram bin.  At most max_out keypoints are written; *n_out
 * receives the number written and *n_dropped (may be NULL) how many more there were (the reference's
 * dropped_features, mod.rs:585).  Host pointers; synchronous. */
int lf_mkd_orient_keypoints(lf_mkd *h, const lf_mkd_extremum *extrema, uint64_t n,
                            lf_mkd_keypoint *out, uint64_t max_out, uint64_t *n_out,
                            uint64_t *n_dropped);

/* Same with DEVICE arrays.  d_frame_of_extremum (may be NULL = frame 0) names each extremum's frame
 * among those given to lf_mkd_set_images_device; d_frame_of_kp (may be NULL) receives the frame of
 * every keypoint written, ready for lf_mkd_describe_keypoints_frames_device.  n_out / n_dropped are
 * HOST pointers: the call waits for `stream` before returning so that the count is valid. */
int lf_mkd_orient_keypoints_device(lf_mkd *h, const lf_mkd_extremum *d_extrema,
                                   const uint32_t *d_frame_of_extremum, uint64_t n,
                                   lf_mkd_keypoint *d_out, uint32_t *d_frame_of_kp, uint64_t max_out,
                                   uint64_t *n_out, uint64_t *n_dropped, void *stream);

/* Detector: the detect task graph after the a-trous stack (swt_sub.glsl, scan_extrema.glsl; constants
 * border = 5, contrast threshold 0.035, skip_layers = 0: mod.rs:76,395-407).  Needs lf_mkd_set_image*.
 * Scans the DoG volume of every loaded frame for 3-D extrema, refines them and applies the edge test;
 * writes {x + dx, y + dy, size, contrast} in a DEFINED order (the reference appends atomically): by frame,
 * then 4x4x4 scan cube in raster order (z, y, x), then position x + 4 y + 16 z in the cube.  A cube keeps at
 * most 8 candidates like the reference, here the first 8 in that order.  At most max_out are written;
 * *n_out = written, *n_dropped (may be NULL) = found beyond max_out (dropped_blobs, mod.rs:625-633).
 * d_frame_of (may be NULL) receives each extremum's frame.  n_out / n_dropped are HOST pointers: waits for
 * `stream`. */
int lf_mkd_detect_extrema_device(lf_mkd *h, lf_mkd_extremum *d_out, uint32_t *d_frame_of, uint64_t max_out,
                                 uint64_t *n_out, uint64_t *n_dropped, void *stream);
int lf_mkd_detect_extrema(lf_mkd *h, lf_mkd_extremum *out, uint64_t max_out, uint64_t *n_out,
                          uint64_t *n_dropped);

/* The host blob filter of detect_top_n on the device (TopKContrastFilter, mod.rs:1753-1786): of the n
 * extrema of ONE frame keep those with size >= min_size and, if more than top_n remain, the top_n with the
 * largest contrast (ties at the cut resolved in index order); index order is preserved.  d_out [top_n]
 * receives the kept extrema, d_index (may be NULL) their indices into d_extrema.  *n_out on the host. */
int lf_mkd_filter_extrema_device(lf_mkd *h, const lf_mkd_extremum *d_extrema, uint64_t n, uint32_t top_n,
                                 float min_size, lf_mkd_extremum *d_out, uint32_t *d_index, uint64_t *n_out,
                                 void *stream);

/* LocalFeaturesVulkan::detect / detect_top_n (mod.rs:346-593) in one call, host pointers, synchronous:
 * image -> pyramid + a-trous stack -> extrema (at most max_blobs) -> [top_n filter if top_n > 0] ->
 * orientation -> sampling -> descriptors.  keypoints [max_out] and descriptors [max_out][128] receive
 * *n_out <= max_out results; *dropped_blobs and *dropped_features (may be NULL) as FeaturesResult
 * (lib.rs:77-83).  max_out beyond 18 x (top_n, or max_blobs when top_n == 0) -- more keypoints than can exist -- is treated as
 * that bound: it sizes no buffer and no copy.  The whole pipeline is one hipGraph launch, recorded the SECOND time these
 * arguments' frame size, top_n, min_size, max_out and pixel type are seen (up to 8 such recordings are kept per handle, the
 * least recently used one makes room): a replayed call costs the upload of the frame, the pipeline and the copy of *n_out
 * results, with one wait in between.  The first sighting of a request is served by the same launches without recording them
 * (one upload, the pipeline's ~20 launches, one wait; same bits) -- the reference's match_images detects each image once, at its
 * own size, and never pays a recording; a camera loop pays it on its second frame (LF_MKD_DETECT_RECORD_AFTER=k in the
 * environment at lf_mkd_create: k sightings before recording, 0 = record at once; cost of the three kinds of call:
 * INTEGRATION.md section 2).  Handles whose keypoint mode takes the two-launch form (LF_MKD_POOL_F32, LF_MKD_POOL_F16_FP6,
 * LF_MKD_FLAG_UNFUSED_KEYPOINTS) always take the stage-by-stage form here.  A frame of 6 MB or more crosses PCIe in pieces
 * (two to four, planned from a model of the link and of the pipeline's front when the request is recorded), and the front --
 * level 0, the a-trous layers, the extremum scan -- runs on the rows a piece completes while the next one is on its way
 * (LF_MKD_DETECT_BANDS=0 in the environment: one piece; LF_MKD_BAND_PIECES=k / LF_MKD_BAND_SPLIT=f1,f2,..: k equal pieces /
 * cuts at these fractions of the height, for tests); same results bit for bit.  Afterwards the handle holds the frame like
 * lf_mkd_set_image.  (benches/bench.rs on houses.jpg, 4096 x 3072, top 2000, n_scales 3: 1.25 ms, 0.91 of it the 50 MB upload
 * at the link's 56 GB/s; lf_mkd_detect_u8 on the same frame: 0.66 ms; n_scales 5: 1.30 / 0.80 ms.) */
int lf_mkd_detect(lf_mkd *h, const float *image, uint32_t width, uint32_t height, uint32_t top_n,
                  float min_size, lf_mkd_keypoint *keypoints, float *descriptors, uint64_t max_out,
                  uint64_t *n_out, uint64_t *dropped_blobs, uint64_t *dropped_features);

/* Host-only diagnostic (needs no device): where lf_mkd_detect / lf_mkd_detect_u8 would cut a frame of this size for its banded
 * upload -- the rows after which a piece ends, ascending, *n_cuts of them (0: one piece; at most max_cuts are written to cuts) --
 * and what the plan's model says: the time (us, from the start of the first copy) at which the pipeline's front has run on the
 * whole frame with these pieces and with one.  bytes_per_pixel 4 (f32 frame) or 1 (8-bit); n_scales as in lf_mkd_params (0: 4).
 * Honours LF_MKD_DETECT_BANDS / LF_MKD_BAND_SPLIT / LF_MKD_BAND_PIECES like the call itself.  modelled_us / one_piece_us may be NULL. */
int lf_mkd_plan_upload(uint32_t width, uint32_t height, uint32_t bytes_per_pixel, uint32_t n_scales, uint32_t *cuts,
                       uint32_t max_cuts, uint32_t *n_cuts, double *modelled_us, double *one_piece_us);

/* lf_mkd_detect on an 8-bit frame (see lf_mkd_set_image_u8): same results, a quarter of the upload. */
int lf_mkd_detect_u8(lf_mkd *h, const uint8_t *image, uint32_t width, uint32_t height, uint32_t top_n, float min_size,
                     lf_mkd_keypoint *keypoints, float *descriptors, uint64_t max_out, uint64_t *n_out,
                     uint64_t *dropped_blobs, uint64_t *dropped_features);

/* detect_top_n over a BATCH of frames (BASELINE configs[2]: hundreds of small frames): n_frames frames of one size,
 * contiguous in device memory, through the whole pipeline with every stage launched once for all frames --
 * pyramids, a-trous stacks, extremum scan, per-frame top_n filter (top_n = 0: every extremum, at most max_blobs
 * per frame), orientation, sampling, description.  Results are ordered by frame, then as lf_mkd_detect orders
 * them; d_frame_of_kp [max_out] names each keypoint's frame.  *dropped_blobs sums the extrema beyond max_blobs
 * over the frames; *dropped_features counts keypoints beyond max_out (a budget for the whole batch).
 * n_frames <= max_frames.  Counts come back to the host (the call waits for `stream`). */
int lf_mkd_detect_frames_device(lf_mkd *h, const float *d_images, uint32_t n_frames, uint32_t width,
                                uint32_t height, uint32_t top_n, float min_size, lf_mkd_keypoint *d_keypoints,
                                uint32_t *d_frame_of_kp, float *d_descriptors, uint64_t max_out,
                                uint64_t *n_out, uint64_t *dropped_blobs, uint64_t *dropped_features,
                                void *stream);

/* Per-frame pipeline as one hipGraph (BASELINE configs[4]: 4K stream, detect + describe per frame).
 * lf_mkd_stream_create records the launch sequence of lf_mkd_detect for frames of width x height -- pyramid,
 * a-trous stack, extremum scan, [top_n filter if top_n > 0], orientation, sampling, description -- with every
 * count handed from stage to stage in device memory, so a frame needs no host round trip.  The buffers are
 * fixed at creation, all DEVICE memory owned by the caller: d_image [height][width] f32 (write the next frame
 * there before each launch), d_keypoints [max_out], d_descriptors [max_out][128], d_counts [8] uint64:
 * [0] extrema found (capped at max_blobs), [1] dropped_blobs, [2] extrema after the top_n filter,
 * [3] keypoints written (valid rows of the two outputs), [4] dropped_features.
 * lf_mkd_stream_frame launches the graph on `stream` (NULL: the handle's stream), asynchronously.
 * One stream pipeline per handle; creating another replaces it.  Creating one also discards the frame loaded by
 * lf_mkd_set_image*: until the first lf_mkd_stream_frame the keypoint, orientation and verification entry points return
 * LF_MKD_ERR_NO_IMAGE; after it they see the frame the pipeline last processed (on the stream it was launched on). */
int lf_mkd_stream_create(lf_mkd *h, uint32_t width, uint32_t height, uint32_t top_n, float min_size,
                         uint64_t max_out, const float *d_image, lf_mkd_keypoint *d_keypoints,
                         float *d_descriptors, uint64_t *d_counts);
int lf_mkd_stream_frame(lf_mkd *h, void *stream);

/* Brute-force matcher: match_features of examples/match_images/src/main.rs:8-27.  For every row of a [na][128]:
 * similarity = dot product with every row of b [nb][128]; best = the largest (the HIGHEST index among equal maxima,
 * as the reference's stable sort leaves it), second = the next one down; match[i] = index of the best if
 * best * ratio > second (the reference uses ratio = 0.8), else -1; ratio <= 0 skips the test and returns the best
 * index as is.  d_best / d_second (may be NULL) receive the two similarities, with which a caller can apply another
 * acceptance rule -- e.g. the webcam example's inner-product-distance form, (1 - best) < 0.75 (1 - second)
 * (examples/webcam/src/main.rs:261-265).  d_exclude_lo / d_exclude_hi (may both be NULL): b rows [lo[i], hi[i]) are not candidates for
 * a row i -- the cross-image form of BASELINE configs[3], where b is the all-gathered descriptor set and a row
 * must not match its own image.  nb must be at least 2 (the reference indexes the second-to-last candidate).
 * Similarities come from the matrix cores in one of three forms, all within ~1e-7 of an f32 dot product, so that decisions
 * can differ from the reference's only where two similarities, or best*ratio and second, agree to that level:
 *   small   -- na * nb <= 2^23 and nb <= 4096 (the reference's own 2000 x 2000): ONE launch straight from the f32 rows, the
 *              scan's three terms formed in registers, no operand tiles and no scratch buffer;
 *   scan    -- every pair from f16 hi+lo splits of both sides (three MFMA terms; ~2^-21 relative for rows of unit norm or
 *              larger -- the lo parts of much smaller elements fall below the f16 grid); ~1.7e12 pairs/s on an MI355X;
 *              used for mid-sized problems;
 *   screen  -- two passes, for na >= 16384 and na * nb >= 2^29: every pair is screened with the f16 roundings of both sides
 *              (one term; error bounded by ~1e-3 |a||b|, from the rows' norms), every candidate within that bound of a row's
 *              second best is re-scored as an f32 dot product, and the decision is taken on the re-scored values: for every
 *              row that is not redone (below), best, second and match are those of an exhaustive scan of b with that dot
 *              product, bit for bit -- 16 partial sums, partial l being a[8l] * b[8l] followed by fmaf(a[8l+j], b[8l+j], .)
 *              for j = 1 .. 7, added as p[l] += p[l ^ 8], then ^ 4, ^ 2, ^ 1, all in f32; the higher index wins among equal
 *              similarities (tests/cpp/match_twin.cpp is that scan on the host); ~5.9e12 pairs/s.  A row with more than 64
 *              such candidates in one lane's share of b (hundreds of near-duplicates of its best match) is redone by the scan
 *              form inside the same call, decided on the device, and carries that form's ~2^-21 instead;
 *              lf_mkd_match_overflowed counts those rows.  (Experiments: LF_MKD_MATCH_SPLITS = b splits;
 *              LF_MKD_MATCH_SHARE = stages between two exchanges of the splits' shared bounds, 0 = none -- 1 publishes the
 *              bounds and never takes them, since a bound is taken one stage after it was asked for.)
 * LF_MKD_MATCH=small, =scan or =screen in the environment forces a form (small: where it fits -- also nb >= 128 or na <= 4096 --
 * else scan).  Elements must be finite and below 65504 in magnitude (f16 range).
 * Device pointers, asynchronous on `stream`.  d_a and d_b must be 16-byte aligned (rows are read as 16-byte vectors; any
 * hipMalloc'd array or row offset into one is: a row is 512 bytes). */
int lf_mkd_match_device(lf_mkd *h, const float *d_a, uint64_t na, const float *d_b, uint64_t nb,
                        const uint32_t *d_exclude_lo, const uint32_t *d_exclude_hi, float ratio,
                        int32_t *d_match, float *d_best, float *d_second, void *stream);
/* Both directions of the reference's example in one call (examples/match_images/src/main.rs:113-116 matches image 1 against
 * image 2 and image 2 against image 1): d_match_ab [na] as lf_mkd_match_device(a, b) gives it, d_match_ba [nb] as
 * lf_mkd_match_device(b, a) does -- decision for decision.  Where both directions fit the one-launch form (the example's own
 * 2000 x 2000) they ARE one launch: the second direction costs no second launch.  Device pointers (16-byte aligned),
 * asynchronous on `stream`.  An empty side (na == 0 or nb == 0) is LF_MKD_OK and writes nothing, as lf_mkd_match_device with
 * na == 0; otherwise na, nb >= 2.  lf_mkd_match_overflowed afterwards reports the rows redone over BOTH directions. */
int lf_mkd_match_both_device(lf_mkd *h, const float *d_a, uint64_t na, const float *d_b, uint64_t nb, float ratio,
                             int32_t *d_match_ab, int32_t *d_match_ba, void *stream);
/* Many image pairs in one call: n_pairs independent match_features problems (examples/match_images/src/main.rs:8-27) in the
 * layout of the batched verifiers below, so that the outputs go into lf_mkd_verify_homography_device /
 * lf_mkd_verify_fundamental_device unchanged.
 *   Pair p is a rows [offsets_a[p], offsets_a[p+1]) against b rows [offsets_b[p], offsets_b[p+1]).  Both offset arrays hold
 *   n_pairs + 1 uint64 entries, live on the device and are non-decreasing.  na_total / nb_total are the numbers of
 *   addressable rows of d_a / d_b (each at most 2^31 - 1): the host sizes the grid from them, never reads the offsets and
 *   never waits.  Rows outside [offsets[0], offsets[n_pairs]) are neither read nor written; whatever the offsets hold, no row
 *   at or beyond a total is touched (an offset beyond the total is read as the total; an inverted pair is an empty one).
 * Outputs: d_match_ab [na_total]: for row i of pair p the index LOCAL to the pair's b rows, or -1.  d_match_ba [nb_total]
 * (may be NULL unless LF_MKD_MATCH_MUTUAL): the other direction, indices local to the pair's a rows.  d_best / d_second
 * [na_total] (may be NULL): the two similarities of the a -> b direction.
 * Per pair: with nb_p >= 2 (and na_p >= 2 for the reverse direction) every output of pair p equals, bit for bit,
 * lf_mkd_match_device on that pair's rows in its one-launch ("small") form -- the same three terms in the same order, best *
 * ratio > second (main.rs:22), ties to the highest index, ratio <= 0: no test.  A side the single-pair call refuses (nb_p < 2,
 * or na_p < 2 for the reverse direction; main.rs:20) yields -1 for every row of that direction and -inf in best / second,
 * whatever the ratio: a batch survives an empty frame.  The result of a pair depends neither on n_pairs, nor on the other
 * pairs, nor on the run.
 * flags: LF_MKD_MATCH_MUTUAL -- both directions are decided with the ratio test; then match_ab[i] = j survives iff
 * match_ba[j] == i, and match_ba[j] = i survives iff match_ab[i] == j (both evaluated on the unfiltered arrays); everything
 * else becomes -1.  d_best / d_second are not filtered.
 * Sizes: any pair size is correct, but every workgroup (16 a rows) converts its pair's whole b side, as the small form does:
 * the call is meant for pairs of up to about 4096 rows per side.  One large pair belongs to lf_mkd_match_device, which picks
 * the scan or screen form for it.
 * One launch (three with LF_MKD_MATCH_MUTUAL), no scratch and no allocation, asynchronous on `stream` (NULL: the handle's
 * own): capturable in a hipGraph.  n_pairs == 0 is LF_MKD_OK and writes nothing.  LF_MKD_ERR_BAD_ARG, reported before any
 * device is touched (the message starts with "match_pairs_device" and is reachable through lf_mkd_last_error(NULL) when h is
 * NULL): a null handle; null d_a, d_b, offsets or d_match_ab; LF_MKD_MATCH_MUTUAL without d_match_ba; unknown flag bits; d_a
 * or d_b not 16-byte aligned; a total above 2^31 - 1; floor(na_total / 16) + n_pairs (plus the same over b when d_match_ba
 * is given) above 2^31 - 1 workgroups.  lf_mkd_match_overflowed afterwards reports 0: this form redoes nothing.
 * (LF_MKD_MATCH_MUTUAL is defined with the verifiers' flag, below their prototypes.) */
int lf_mkd_match_pairs_device(lf_mkd *h, const float *d_a, const uint64_t *d_offsets_a, uint64_t na_total,
                              const float *d_b, const uint64_t *d_offsets_b, uint64_t nb_total, uint32_t n_pairs,
                              float ratio, uint32_t flags, int32_t *d_match_ab, int32_t *d_match_ba, float *d_best,
                              float *d_second, void *stream);
/* Guided matching: lf_mkd_match_pairs_device once more, under each pair's verified model.  Once lf_mkd_verify_homography_device
 * or lf_mkd_verify_fundamental_device has given pair p its H or F, the ratio test is run again over only the candidates the
 * geometry allows: the rows of the other side inside a transfer disc (H) or an epipolar band (F).  That recovers matches which
 * the unrelated rows of a whole frame suppressed, and the second best is then a competitor in the same place.
 *   Layout, offset rules, outputs and LF_MKD_MATCH_MUTUAL are exactly those of lf_mkd_match_pairs_device: offsets on the device
 *   and never read by the host; an offset beyond a total is read as the total, an inverted pair is empty; match values are
 *   local to the pair; rows outside the pairs are untouched.  d_kps_a [na_total] / d_kps_b [nb_total] are indexed like the
 *   descriptor rows; only x and y are read.  d_model is [n_pairs][9] floats, exactly what the verifiers write as d_H / d_F.
 * Candidates: row j of pair p's b side is admissible for row i of its a side iff the verifier's own step-4 test (below) holds
 * for the point pair (a_i, b_j) with thr2 = threshold_px * threshold_px formed as the verifiers form it -- the same correctly
 * rounded operations in the same order:
 *   LF_MKD_GUIDE_HOMOGRAPHY   u, v, w = H a;  w > 0  and  fmaf(ex, ex, ey * ey) < thr2 * (w * w),  ex = fmaf(bx, w, -u), ey likewise
 *   LF_MKD_GUIDE_FUNDAMENTAL  the Sampson test  e^2 < thr2 * (l0^2 + l1^2 + l'0^2 + l'1^2),  l = F a, l' = F^T b, e = b . l
 * Both directions use the SAME relation: the candidates of b row j in the b -> a direction are the a rows i with
 * admissible(a_i, b_j); no inverse model is formed, so the relation is symmetric by construction and the mutual rule
 * meaningful.  An all-zero model (what verification writes when it found nothing), a NaN anywhere in the model and a NaN
 * coordinate need no special case: the comparison is false, the row has no candidate.
 * Decision, per row: best and second are the largest and the next similarity over the admissible rows ONLY -- the one-launch
 * form's similarity, the same three terms in the same order, ties to the highest index; match = the best's index if
 * ratio <= 0 or best * ratio > second, else -1.  A row with one candidate has second = -inf and is accepted; a row with none
 * gets -1 and -inf in both scores.  There is no refusal of a small side here (nb_p < 2 is fine): one row is a legitimate
 * candidate set.  The result of a pair depends neither on n_pairs, nor on the other pairs, nor on the run.
 * Superset property: take `verified` from lf_mkd_verify_*_device run on the LF_MKD_MATCH_MUTUAL output of
 * lf_mkd_match_pairs_device; run this call with that model, the same kind, the same ratio, LF_MKD_MATCH_MUTUAL and a
 * threshold not below the verifier's.  Then every verified[i] = j >= 0 has match_ab[i] == j and match_ba[j] == i: j was i's
 * best over a superset of the admissible rows, with ties to the highest index, so it is the best of the subset; the subset's
 * second is not above the superset's, so the ratio test still passes; the reverse direction likewise; and thr2 * den is
 * monotone in thr2, so an inlier of the verifier is admissible here.  Guided matching never loses a verified match.
 * Cost: a 16 x 16 tile of candidates is tested on 8 bytes per row before any of its descriptors is requested, and a tile
 * without an admissible pair is skipped whole -- under a homography, almost every tile.
 * One launch (three with LF_MKD_MATCH_MUTUAL), no scratch and no allocation, asynchronous on `stream` (NULL: the handle's own):
 * capturable in a hipGraph.  n_pairs == 0 is LF_MKD_OK and writes nothing.  LF_MKD_ERR_BAD_ARG, reported before any device is
 * touched (the message starts with "match_guided_pairs_device" and is reachable through lf_mkd_last_error(NULL) when h is
 * NULL): a null handle; null d_a, d_b, d_kps_a, d_kps_b, offsets, d_model or d_match_ab; LF_MKD_MATCH_MUTUAL without
 * d_match_ba; unknown flag bits; kind > 1; threshold_px not positive or its f32 square not a finite normal number (the
 * verifiers' rule); d_a or d_b not 16-byte aligned; a total above 2^31 - 1; floor(na_total / 16) + n_pairs (plus the same
 * over b when d_match_ba is given) above 2^31 - 1 workgroups.
 * (LF_MKD_GUIDE_* and LF_MKD_MATCH_MUTUAL are defined with the verifiers' flag, below their prototypes.) */
int lf_mkd_match_guided_pairs_device(lf_mkd *h, const float *d_a, const lf_mkd_keypoint *d_kps_a,
                                     const uint64_t *d_offsets_a, uint64_t na_total, const float *d_b,
                                     const lf_mkd_keypoint *d_kps_b, const uint64_t *d_offsets_b, uint64_t nb_total,
                                     const float *d_model, uint32_t n_pairs, uint32_t kind, float threshold_px, float ratio,
                                     uint32_t flags, int32_t *d_match_ab, int32_t *d_match_ba, float *d_best,
                                     float *d_second, void *stream);
/* Host pointers, synchronous. */
int lf_mkd_match(lf_mkd *h, const float *a, uint64_t na, const float *b, uint64_t nb, float ratio,
                 int32_t *match);
/* Diagnostic: *n_rows = rows of a that the handle's latest match call had to redo by the full scan (0 in the ordinary
 * case).  Waits for that call to finish (synchronises `stream`, NULL = the handle's own). */
int lf_mkd_match_overflowed(lf_mkd *h, void *stream, uint64_t *n_rows);

/* ---- 8-bit descriptors: the quantiser and the exact int8 matcher -------------------------------------------------
 * The format.  A quantised descriptor is 128 uint8_t (128 bytes a row instead of 512), offset-binary: byte = q + 128 with
 * q in [-127, 127], so bytes are 1 .. 255 and 0 never occurs.  q = clamp(rint(x * scale), -127, 127): x * scale is one
 * correctly rounded f32 multiplication, rint rounds to nearest with ties to even, a NaN product gives q = 0, +-inf
 * saturates.  `scale` is a call argument, a positive, finite, normal f32; 0 means the default, 256.  The descriptors are
 * L2-normalised, so |x| <= 1 and in practice far below it: at 256 nothing below |x| = 0.496 saturates.  Unsigned on the
 * boundary because uint8 is what every binding has; the matcher turns a dword of it into two's complement with one xor
 * 0x80808080.  One global scale, not one per row: the rows have unit norm, and a per-row scale would make the similarities
 * of one a row against different b rows incomparable as integers.  With s the integer similarity below, s / scale^2
 * approximates the f32 dot product; for two rows without a saturated element
 *   |s / scale^2 - <a, b>| <= (|a|_1 + |b|_1) / (2 scale) + 128 / (4 scale^2).
 *
 * lf_mkd_quantize_descriptors_device: d_desc [n][128] f32 -> d_q [n][128] bytes, exactly n * 128 bytes written.  Device
 * pointers (d_desc 16-byte, d_q 4-byte aligned), one launch, asynchronous on `stream` (NULL: the handle's own), no scratch:
 * capturable in a hipGraph.  n == 0 is LF_MKD_OK and writes nothing.  lf_mkd_quantize_descriptors is the same for host
 * pointers (any alignment), synchronous, through the handle's staging.
 * LF_MKD_ERR_BAD_ARG, reported before any device is touched (the message starts with "quantize_descriptors_device" /
 * "quantize_descriptors" and is reachable through lf_mkd_last_error(NULL) when h is NULL): a null handle; with n > 0 a null
 * or misaligned pointer; n above 2^31 - 1; a scale that is negative, NaN, infinite or subnormal. */
int lf_mkd_quantize_descriptors_device(lf_mkd *h, const float *d_desc, uint64_t n, float scale, uint8_t *d_q,
                                       void *stream);
int lf_mkd_quantize_descriptors(lf_mkd *h, const float *desc, uint64_t n, float scale, uint8_t *q);
/* The matcher over quantised rows: lf_mkd_match_device's semantics restated for integers, and exact.
 *   similarity  s(i, j) = sum_k (a[i][k] - 128) * (b[j][k] - 128), an exact int32 (|s| <= 128 * 127^2 = 2 064 512 < 2^24);
 *   best        the largest s over the candidates; among equal maxima the HIGHEST index wins;
 *   second      the largest over the remaining candidates (equal to best when the maximum occurs twice);
 *   exclusion   b rows [lo[i], hi[i]) are not candidates for a row i (both pointers NULL: none; one NULL: refused);
 *   acceptance  match[i] = the best's index if ratio <= 0 or (float)best * ratio > (float)second -- both conversions are
 *               exact, one f32 multiplication -- else -1;
 *   too few     with one candidate second = INT32_MIN and the row is accepted; with none match = -1 and best = second =
 *               INT32_MIN.
 * d_best / d_second [na] int32 may be NULL.  nb must be at least 2, as in the f32 call; na == 0 is LF_MKD_OK and writes
 * nothing.  d_a and d_b must be 16-byte aligned (a row is 128 bytes).  The result depends on the inputs alone: not on the
 * run, not on the split count, not on the device's CU count -- integer sums have no rounding, every tie rule is by index.
 * There is one form for every size (v_mfma_i32_32x32x32_i8, 4 matrix instructions per 32 x 32 tile of pairs, b streamed
 * through LDS straight from the caller's rows): no operand tiles, no margin, no re-score, no fallback, and
 * lf_mkd_match_overflowed is not affected.  Two launches (scan over a grid of a blocks x b splits, then a merge of the
 * splits' partial results), one when the plan below has one split.  Asynchronous on `stream` (NULL: the handle's own), no
 * host synchronisation, no allocation once the handle's scratch (the splits' partials) has grown to the largest plan seen;
 * a warmed-up call can be captured in a hipGraph.  lf_mkd_match_q8 is the same for host pointers, synchronous, without
 * exclusion ranges.
 * LF_MKD_ERR_BAD_ARG, reported before any device is touched (the message starts with "match_q8_device" / "match_q8" and is
 * reachable through lf_mkd_last_error(NULL) when h is NULL): a null handle; with na > 0 a null d_a, d_b or d_match; one
 * exclusion pointer without the other; d_a or d_b not 16-byte aligned; nb < 2; na or nb above 2^31 - 1. */
int lf_mkd_match_q8_device(lf_mkd *h, const uint8_t *d_a, uint64_t na, const uint8_t *d_b, uint64_t nb,
                           const uint32_t *d_exclude_lo, const uint32_t *d_exclude_hi, float ratio, int32_t *d_match,
                           int32_t *d_best, int32_t *d_second, void *stream);
int lf_mkd_match_q8(lf_mkd *h, const uint8_t *a, uint64_t na, const uint8_t *b, uint64_t nb, float ratio,
                    int32_t *match);
/* What lf_mkd_match_q8_device launches for a problem size, and the scratch it needs -- host-only, no device, no handle, no
 * environment variable; the launch path calls this very function.  num_cus: the device's compute units, 0 means 256.
 * *a_blocks x *b_splits is the scan's grid: an a block is 1024 rows (8 waves x 4 tiles of 32), a split a contiguous range of
 * 32-row b tiles.  b_splits is 1 when all of b is one LDS stage (nb <= 128); otherwise about two workgroups per CU, at least
 * 2 and at most one per b tile (and at most 1024) -- a condition on nb alone.  *scratch_bytes is 0 exactly when b_splits == 1
 * (the scan then writes the result itself) and otherwise 12 bytes per (split, a row), stated as an upper bound that is
 * non-decreasing in na for a given nb and num_cus and within a factor 2 of b_splits * na * 12:
 *   12 * 1024 * min(A + max(W, A), A * ceil(nb / 32)),  A = a_blocks, W = 2 * num_cus.
 * na == 0: (0, 1, 0).  Output pointers may be NULL.  LF_MKD_ERR_BAD_ARG (message "match_q8_plan: ...", through
 * lf_mkd_last_error(NULL)): nb < 2, na or nb above 2^31 - 1. */
int lf_mkd_match_q8_plan(uint64_t na, uint64_t nb, uint32_t num_cus, uint32_t *a_blocks, uint32_t *b_splits,
                         uint64_t *scratch_bytes);
/* k-nearest-neighbour search over quantised rows: each a row's k best b rows, exact.
 *   Rows, similarity and exclusion are lf_mkd_match_q8_device's, word for word: rows are 128 offset-binary bytes; s(i, j) is
 *   the exact int32 sum; b rows [lo[i], hi[i]) are not candidates of a row i (both pointers NULL: none; one NULL: refused); an
 *   inverted or empty range excludes nothing; a bound beyond nb is read as nb.
 *   order       a row's candidates are totally ordered: larger s first, and among equal s the HIGHER index first;
 *   output      d_index[i * k + c] / d_score[i * k + c], c = 0 .. k - 1, are the first k candidates of row i in that order;
 *               slots beyond the number of candidates hold -1 / INT32_MIN.  Exactly na * k entries of each array are
 *               written.  d_score may be NULL.
 *   matcher     column 0 is what lf_mkd_match_q8_device returns with ratio <= 0 (its index and its best) and column 1's
 *               score is its second -- by construction: that call's best is the first candidate of this order and its
 *               second the score of the next one, so second == best when the maximum occurs twice falls out of the order.
 * 1 <= k <= LF_MKD_KNN_MAX.  nb >= 1: one candidate is a legitimate answer here, unlike the ratio-test call.  na == 0 is
 * LF_MKD_OK and writes nothing.  na and nb are at most 2^31 - 1.  d_a and d_b must be 16-byte aligned, d_index and d_score
 * 4-byte aligned.  The result depends on the inputs alone: not on the run, not on the split count, not on the device's CU
 * count -- a candidate is one 64-bit key (s + 2^21) << 32 | index, keys are unique per row, and every step is a max-merge of
 * keys.
 * One launch (the scan over a grid of a blocks x b splits) or two (a merge of the splits' lists when the plan below has more
 * than one split).  Asynchronous on `stream` (NULL: the handle's own), no host synchronisation, no allocation once the
 * handle's q8 scratch has grown to the largest plan seen; a warmed-up call can be captured in a hipGraph.  The scratch is the
 * one lf_mkd_match_q8_device uses, so the calls of one handle must be stream-ordered, as that call already requires.
 * lf_mkd_match_overflowed is not affected.  lf_mkd_knn_q8 is the same for host pointers (any alignment), synchronous, without
 * exclusion ranges, through the handle's staging; `score` may be NULL.
 * LF_MKD_ERR_BAD_ARG, reported before any device is touched (the message starts with "knn_q8_device: " / "knn_q8: " and is
 * reachable through lf_mkd_last_error(NULL) when h is NULL): a null handle; with na > 0 a null d_a, d_b or d_index; one
 * exclusion pointer without the other; d_a or d_b not 16-byte aligned; k == 0 or k > LF_MKD_KNN_MAX (the message names k);
 * nb == 0; na or nb above 2^31 - 1. */
#define LF_MKD_KNN_MAX (16)
int lf_mkd_knn_q8_device(lf_mkd *h, const uint8_t *d_a, uint64_t na, const uint8_t *d_b, uint64_t nb,
                         const uint32_t *d_exclude_lo, const uint32_t *d_exclude_hi, uint32_t k, int32_t *d_index,
                         int32_t *d_score, void *stream);
int lf_mkd_knn_q8(lf_mkd *h, const uint8_t *a, uint64_t na, const uint8_t *b, uint64_t nb, uint32_t k, int32_t *index,
                  int32_t *score);
/* What lf_mkd_knn_q8_device launches for a problem size, and the scratch it needs -- host-only, no device, no handle, no
 * environment variable; the launch path calls this very function.  num_cus: the device's compute units, 0 means 256.
 * *a_blocks x *b_splits is the scan's grid: an a block is 256 rows (8 waves x 1 tile of 32), a split a contiguous range of
 * 32-row b tiles, none empty.  b_splits is 1 when all of b is one LDS stage (nb <= 128); otherwise about two workgroups per
 * CU, at least 2 and at most one per b tile (and at most 1024) -- a condition on nb alone.  *scratch_bytes is 0 exactly when
 * b_splits == 1 (the scan then writes the result itself) and otherwise 8 k bytes per (split, a row), stated as an upper
 * bound that is non-decreasing in na for a given nb, k and num_cus (a handle warmed up on its largest problem never
 * allocates again):
 *   8 k * 256 * min(A + max(W, A), A * ceil(nb / 32)),  A = a_blocks, W = 2 * num_cus.
 * na == 0: (0, 1, 0).  Output pointers may be NULL.  LF_MKD_ERR_BAD_ARG (message "knn_q8_plan: ...", through
 * lf_mkd_last_error(NULL)): k == 0 or k > LF_MKD_KNN_MAX, nb == 0, na or nb above 2^31 - 1. */
int lf_mkd_knn_q8_plan(uint64_t na, uint64_t nb, uint32_t k, uint32_t num_cus, uint32_t *a_blocks, uint32_t *b_splits,
                       uint64_t *scratch_bytes);
/* Grouped matching over quantised rows: the ratio test against the best neighbour from ANOTHER group (image, object,
 * landmark) -- Lowe's object-recognition rule for a pooled database, exact.
 *   Rows, similarity and exclusion are lf_mkd_match_q8_device's, word for word: rows are 128 offset-binary bytes; s(i, j) is
 *   the exact int32 sum; b rows [lo[i], hi[i]) are not candidates of a row i (both pointers NULL: none; one NULL: refused); an
 *   inverted or empty range excludes nothing; a bound beyond nb is read as nb.
 *   groups      d_group_of_b[j] is any uint32, the group of b row j.  The ids need not be sorted, dense or contiguous: only
 *               the equality of two ids is ever used.
 *   order       a row's candidates are totally ordered as in lf_mkd_knn_q8_device: larger s first, and among equal s the
 *               HIGHER index first.
 *   output      d_best[i] is the score of the first candidate of that order and its index is the row's match; d_rival[i] is
 *               the score of the first candidate of that order whose group differs from the best's group, INT32_MIN if there
 *               is none.  d_match[i] is the best's index if  ratio <= 0 || (float)best * ratio > (float)rival,  else -1: both
 *               conversions are exact and there is one f32 multiplication.  A row without a candidate gets -1 and INT32_MIN in
 *               both scores.  Exactly na entries of each array are written.  d_best and d_rival may be NULL.
 * By construction:
 *   (a) with d_group_of_b[j] = j every output equals lf_mkd_match_q8_device's, with rival == second;
 *   (b) with all groups equal, rival == INT32_MIN and every row with a candidate is accepted at any ratio;
 *   (c) best and, at ratio 0, match are column 0 of lf_mkd_knn_q8_device; rival is the score of the first of that call's
 *       columns whose row has another group than column 0's, whenever there is one among the k.
 * nb >= 1: a pool of one row, or of one group, is a legitimate question here, as in the top-k call.  na == 0 is LF_MKD_OK and
 * writes nothing.  na and nb are at most 2^31 - 1.  d_a and d_b must be 16-byte aligned, the other arrays 4-byte aligned.
 * The result depends on the inputs alone: not on the run, not on the split count, not on the device's CU count -- a row's
 * state is (best, index, group of best, rival), and two states over disjoint row sets merge exactly: the one with the larger
 * (best, index) wins and its rival becomes the maximum of its own and, if the best groups differ, the loser's best, else the
 * loser's rival.
 * One launch (the scan over a grid of a blocks x b splits) or two (a merge of the splits' states when the plan below has more
 * than one split).  Asynchronous on `stream` (NULL: the handle's own), no host synchronisation, no allocation once the
 * handle's q8 scratch has grown to the largest plan seen; a warmed-up call can be captured in a hipGraph.  The scratch is the
 * one lf_mkd_match_q8_device and lf_mkd_knn_q8_device use, so the calls of one handle must be stream-ordered, as those calls
 * already require.  lf_mkd_match_overflowed is not affected.  lf_mkd_match_q8_grouped is the same for host pointers (any
 * alignment), synchronous, without exclusion ranges, through the handle's staging; `best` and `rival` may be NULL.
 * Cost: group ids are read only for the candidates that pass the top-2 code's gate (a tile's maximum above the rival or at
 * least the best).  With a SINGLE group nothing ever raises the rival, so that gate never closes and every tile pays the
 * update: such a pool belongs to lf_mkd_match_q8_device at ratio 0.
 * LF_MKD_ERR_BAD_ARG, reported before any device is touched (the message starts with "match_q8_grouped_device: " /
 * "match_q8_grouped: " and is reachable through lf_mkd_last_error(NULL) when h is NULL): a null handle; with na > 0 a null
 * d_a, d_b, d_group_of_b or d_match; one exclusion pointer without the other; d_a or d_b not 16-byte aligned or another array
 * not 4-byte aligned; nb == 0; na or nb above 2^31 - 1. */
int lf_mkd_match_q8_grouped_device(lf_mkd *h, const uint8_t *d_a, uint64_t na, const uint8_t *d_b, uint64_t nb,
                                   const uint32_t *d_group_of_b, const uint32_t *d_exclude_lo, const uint32_t *d_exclude_hi,
                                   float ratio, int32_t *d_match, int32_t *d_best, int32_t *d_rival, void *stream);
int lf_mkd_match_q8_grouped(lf_mkd *h, const uint8_t *a, uint64_t na, const uint8_t *b, uint64_t nb,
                            const uint32_t *group_of_b, float ratio, int32_t *match, int32_t *best, int32_t *rival);
/* What lf_mkd_match_q8_grouped_device launches for a problem size, and the scratch it needs -- host-only, no device, no
 * handle, no environment variable; the launch path calls this very function.  num_cus: the device's compute units, 0 means
 * 256.  *a_blocks x *b_splits is the scan's grid: an a block is 256 rows (8 waves x 1 tile of 32), a split a contiguous range
 * of 32-row b tiles, none empty.  b_splits is 1 when all of b is one LDS stage (nb <= 128); otherwise about two workgroups per
 * CU, at least 2 and at most one per b tile (and at most 1024) -- a condition on nb alone.  *scratch_bytes is 0 exactly when
 * b_splits == 1 (the scan then writes the result itself) and otherwise 16 bytes per (split, a row), stated as an upper bound
 * that is non-decreasing in na for a given nb and num_cus (a handle warmed up on its largest problem never allocates again):
 *   16 * 256 * min(A + max(W, A), A * ceil(nb / 32)),  A = a_blocks, W = 2 * num_cus.
 * na == 0: (0, 1, 0).  Output pointers may be NULL.  LF_MKD_ERR_BAD_ARG (message "match_q8_grouped_plan: ...", through
 * lf_mkd_last_error(NULL)): nb == 0, na or nb above 2^31 - 1. */
int lf_mkd_match_q8_grouped_plan(uint64_t na, uint64_t nb, uint32_t num_cus, uint32_t *a_blocks, uint32_t *b_splits,
                                 uint64_t *scratch_bytes);
/* The group-by-group vote table of a match array: the second half of retrieval, on the device.
 *   d_votes is [n_groups_a][n_groups_b] uint32; exactly that many entries are written (the call zeroes them first).
 *   votes[ga][gb] is the number of rows i with  0 <= d_match[i] < nb,  ga = d_group_of_a[i] < n_groups_a  (d_group_of_a NULL:
 *   ga = 0 for every row) and  gb = d_group_of_b[d_match[i]] < n_groups_b.  Rows failing any of the three are not counted;
 *   nothing is read out of range.
 * Integer atomic adds, so the table does not depend on the order.  Two launches (the zeroing is a kernel, not a memset: a
 * captured memset node of this size was seen to replay a stale fill pattern on ROCm 7.2), asynchronous on `stream` (NULL:
 * the handle's own), no scratch, capturable.  LF_MKD_ERR_BAD_ARG before any device is touched (message
 * "vote_groups_device: ...", through lf_mkd_last_error(NULL) when h is NULL): a null handle; with na > 0 a null d_match or
 * d_group_of_b; a null d_votes; a group count of zero; n_groups_a * n_groups_b above 2^31 - 1; na or nb above 2^31 - 1; an
 * array that is not 4-byte aligned. */
int lf_mkd_vote_groups_device(lf_mkd *h, const int32_t *d_match, uint64_t na, const uint32_t *d_group_of_a, uint32_t n_groups_a,
                              const uint32_t *d_group_of_b, uint64_t nb, uint32_t n_groups_b, uint32_t *d_votes, void *stream);
/* Many pairs of 8-bit rows in one call: lf_mkd_match_pairs_device over the q8 format above, for the multi-frame pipeline.
 *   Layout and offsets are those of lf_mkd_match_pairs_device, word for word: pair p is a rows [offsets_a[p], offsets_a[p+1])
 *   against b rows [offsets_b[p], offsets_b[p+1]); both offset arrays hold n_pairs + 1 uint64 entries, live on the device, are
 *   non-decreasing and are never read by the host.  An offset beyond a total is read as the total; an inverted pair is empty;
 *   no row at or beyond a total is read or written; rows outside [offsets[0], offsets[n_pairs]) are neither read nor written.
 *   Rows are 128 offset-binary bytes; d_a and d_b must be 16-byte aligned.
 * Per pair: with nb_p >= 2 (and na_p >= 2 for the reverse direction) every output of pair p EQUALS what
 * lf_mkd_match_q8_device writes for that pair's rows alone without exclusion ranges -- exact integer similarity, ties to the
 * highest index, second == best when the maximum occurs twice, acceptance ratio <= 0 || (float)best * ratio > (float)second.
 * d_match_ab [na_total] / d_match_ba [nb_total] are local to the pair; d_best / d_second [na_total] are the int32 sums of the
 * a -> b direction and may be NULL.  A side with too few candidates (nb_p < 2, or na_p < 2 for the reverse direction) yields
 * -1 for every row of that direction and INT32_MIN in best / second, whatever the ratio: a batch survives an empty frame.
 * The result of a pair depends neither on n_pairs, nor on the other pairs, nor on the run, nor on the device's CU count.
 * d_match_ba may be NULL unless LF_MKD_MATCH_MUTUAL is set; when given, both directions are decided in the same matcher
 * launch.  LF_MKD_MATCH_MUTUAL then keeps match_ab[i] = j iff match_ba[j] == i and match_ba[j] = i iff match_ab[i] == j (both
 * evaluated on the unfiltered arrays; two element-wise launches); d_best / d_second are not filtered.
 * Sizes: any pair size is correct, but every workgroup (*block_rows a rows, below) streams its pair's whole b side through
 * LDS: the call is meant for pairs of up to about 4096 rows per side.  One large pair belongs to lf_mkd_match_q8_device.
 * One launch (three with LF_MKD_MATCH_MUTUAL), no scratch (the handle's q8 scratch is not touched), no allocation, no host
 * synchronisation, asynchronous on `stream` (NULL: the handle's own): capturable in a hipGraph.  n_pairs == 0 is LF_MKD_OK
 * and writes nothing.  lf_mkd_match_overflowed is not affected.
 * LF_MKD_ERR_BAD_ARG, reported before any device is touched (the message starts with "match_q8_pairs_device" and is
 * reachable through lf_mkd_last_error(NULL) when h is NULL): a null handle; null d_a, d_b, offsets or d_match_ab;
 * LF_MKD_MATCH_MUTUAL without d_match_ba; unknown flag bits; d_a or d_b not 16-byte aligned; a total above 2^31 - 1; a grid
 * (the plan below, with both_directions = d_match_ba given) above 2^31 - 1 workgroups. */
int lf_mkd_match_q8_pairs_device(lf_mkd *h, const uint8_t *d_a, const uint64_t *d_offsets_a, uint64_t na_total,
                                 const uint8_t *d_b, const uint64_t *d_offsets_b, uint64_t nb_total, uint32_t n_pairs,
                                 float ratio, uint32_t flags, int32_t *d_match_ab, int32_t *d_match_ba,
                                 int32_t *d_best, int32_t *d_second, void *stream);
/* Guided matching over 8-bit rows: lf_mkd_match_q8_pairs_device once more, under each pair's verified model -- the conjunction
 * of that call's contract and lf_mkd_match_guided_pairs_device's.  A caller who quantised once and dropped the f32 rows can
 * run the pass behind verification on the bytes.
 *   Layout, offsets, outputs and LF_MKD_MATCH_MUTUAL are those of lf_mkd_match_q8_pairs_device: pair p is a rows
 *   [offsets_a[p], offsets_a[p+1]) against b rows [offsets_b[p], offsets_b[p+1]); both offset arrays hold n_pairs + 1 uint64
 *   entries, live on the device, are non-decreasing and are never read by the host.  An offset beyond a total is read as the
 *   total; an inverted pair is empty; match values are local to the pair; no row at or beyond a total is read or written; rows
 *   outside [offsets[0], offsets[n_pairs]) are neither read nor written.  Rows are 128 offset-binary bytes; d_a and d_b must be
 *   16-byte aligned.  d_best / d_second [na_total] are the int32 sums of the a -> b direction and may be NULL.
 *   Keypoints and model are those of lf_mkd_match_guided_pairs_device: d_kps_a [na_total] / d_kps_b [nb_total] are indexed like
 *   the descriptor rows, only x and y are read; d_model is [n_pairs][9] floats, exactly what the verifiers write as d_H / d_F.
 * Candidates: that call's relation, bit for bit.  Row j of pair p's b side is admissible for row i of its a side iff the
 * verifier's own step-4 test holds for the point pair (a_i, b_j) with thr2 = threshold_px * threshold_px formed on the host
 * as the verifiers form it (LF_MKD_GUIDE_HOMOGRAPHY: w > 0 and fmaf(ex, ex, ey * ey) < thr2 * (w * w); LF_MKD_GUIDE_FUNDAMENTAL:
 * the Sampson test -- the same correctly rounded operations in the same order, stated above).  Both directions evaluate
 * pred(a_i, b_j); no inverse model is formed.  An all-zero model, a NaN anywhere in the model and a NaN coordinate need no
 * special case: the comparison is false, the row has no candidate.
 * Decision, per row: lf_mkd_match_q8_device's over the admissible rows ONLY -- the similarity is the exact int32 sum; ties go
 * to the highest index; second == best when the maximum occurs twice among the admissible rows; match = the best's index if
 * ratio <= 0 || (float)best * ratio > (float)second, else -1.  A row with one candidate has second = INT32_MIN and is
 * accepted; a row with none gets -1 and INT32_MIN in both scores.  A small side is not refused here: nb_p == 1 is a legitimate
 * candidate set, as in the f32 guided call (the unguided q8 pairs call refuses nb_p < 2; this one does not).  The result of a
 * pair depends on its inputs alone: not on n_pairs, not on the other pairs, not on the run, not on the device's CU count.
 * Superset property: take `verified` from lf_mkd_verify_*_device run on the LF_MKD_MATCH_MUTUAL output of
 * lf_mkd_match_q8_pairs_device; run this call with that model, the same kind, the same ratio, LF_MKD_MATCH_MUTUAL and a
 * threshold not below the verifier's.  Then every verified[i] = j >= 0 has match_ab[i] == j and match_ba[j] == i: j was i's
 * best over a superset of the admissible rows, with ties to the highest index, so it is the best of the subset (the sums are
 * the same integers in both calls); the subset's second is not above the superset's, and int32 -> f32 is monotone, so
 * (float)best * ratio > (float)second still holds -- or ratio <= 0 held already; the reverse direction likewise; and
 * thr2 * den is monotone in thr2, so an inlier of the verifier is admissible here.  (A verified match implies nb_p >= 2 and
 * na_p >= 2: the unguided call accepted it.)  Guided matching never loses a verified match.
 * Cost: every workgroup streams its pair's whole b side through LDS as the unguided call does; a 32 x 32 tile of candidates
 * is tested on its rows' keypoints first, and a tile without an admissible pair costs no matrix instruction.
 * One launch (three with LF_MKD_MATCH_MUTUAL: the two extra are lf_mkd_match_pairs_device's filter), no scratch, no
 * allocation, no host synchronisation, asynchronous on `stream` (NULL: the handle's own): capturable in a hipGraph.
 * n_pairs == 0 is LF_MKD_OK and writes nothing.  The grid is exactly what lf_mkd_match_q8_pairs_plan reports (the same R, the
 * same slot map, both_directions = d_match_ba given).  lf_mkd_match_overflowed is not affected.
 * LF_MKD_ERR_BAD_ARG, reported before any device is touched (the message starts with "match_q8_guided_pairs_device" and is
 * reachable through lf_mkd_last_error(NULL) when h is NULL): a null handle; null d_a, d_b, d_kps_a, d_kps_b, offsets, d_model
 * or d_match_ab; LF_MKD_MATCH_MUTUAL without d_match_ba; unknown flag bits; kind > 1; threshold_px not positive or its f32
 * square not a finite normal number (the verifiers' rule); d_a or d_b not 16-byte aligned; a total above 2^31 - 1; a grid (the
 * plan below) above 2^31 - 1 workgroups. */
int lf_mkd_match_q8_guided_pairs_device(lf_mkd *h, const uint8_t *d_a, const lf_mkd_keypoint *d_kps_a,
                                        const uint64_t *d_offsets_a, uint64_t na_total, const uint8_t *d_b,
                                        const lf_mkd_keypoint *d_kps_b, const uint64_t *d_offsets_b, uint64_t nb_total,
                                        const float *d_model, uint32_t n_pairs, uint32_t kind, float threshold_px, float ratio,
                                        uint32_t flags, int32_t *d_match_ab, int32_t *d_match_ba, int32_t *d_best,
                                        int32_t *d_second, void *stream);
/* The grid lf_mkd_match_q8_pairs_device launches -- host-only, no device, no handle, no environment variable; the launch path
 * calls this very function.  *block_rows = R, the a rows one workgroup owns (a power of two; a build-time constant);
 * *workgroups = floor(na_total / R) + n_pairs, plus floor(nb_total / R) + n_pairs when both_directions != 0.  Output pointers
 * may be NULL.  LF_MKD_ERR_BAD_ARG (message "match_q8_pairs_plan: ...", through lf_mkd_last_error(NULL)): a total above
 * 2^31 - 1, or more than 2^31 - 1 workgroups. */
int lf_mkd_match_q8_pairs_plan(uint64_t na_total, uint64_t nb_total, uint32_t n_pairs, uint32_t both_directions,
                               uint32_t *block_rows, uint64_t *workgroups);
/* ---- edge lists: any pairs of images from one pool, over 8-bit rows, no row copied -------------------------------
 * The pair layout above gives every image to one pair.  A window wider than one, exhaustive matching of N images, a query
 * against its ranked candidates and loop-closure candidates all put one image on MANY pairs; these three calls take such a
 * batch as a list of edges over a pool.
 *   pool        one row array plus d_image_offsets (uint64 [n_images + 1], on the device, never read by the host): image m owns
 *               rows [image_offsets[m], image_offsets[m+1]).  An offset beyond the pool's total is read as the total and an
 *               inverted range is empty, as for a pair; rows that belong to no image are never read.
 *   edge        edge e is (d_edge_a[e], d_edge_b[e]), two uint32 image ids on the device: image edge_a[e] of the a pool against
 *               image edge_b[e] of the b pool.  The two pools are separate arguments and may be the same arrays.  A self edge, a
 *               repeated edge and (j, i) beside (i, j) are ordinary edges.  An id at or beyond n_images names an empty image.
 *   edge layout of one side: an ordinary pair layout, d_edge_offsets (uint64 [n_edges + 1]) with edge_offsets[e+1] -
 *               edge_offsets[e] = the rows of that side's image of edge e.  Everything that is indexed "like a" -- match, best,
 *               second, verified, the keypoints of the rows -- lives in it, so LF_MKD_MATCH_MUTUAL, both verifiers and the
 *               guided calls take (edge_offsets_a, edge_offsets_b) as their offsets, unchanged.
 *
 * lf_mkd_edge_layout_device writes the layout of one side (call it once per side): d_edge_offsets[0] = 0 and
 * d_edge_offsets[e+1] = d_edge_offsets[e] + rows(d_edge_image[e]), where rows(m) is image m's row count against n_rows_total
 * for m < n_images and 0 for any other id.  Exactly n_edges + 1 entries are written; n_edges == 0 is LF_MKD_OK and writes
 * nothing.  Integer sums: the result is exact.  Two launches (one up to 1024 edges), no scratch, no allocation, no host
 * synchronisation, asynchronous on `stream` (NULL: the handle's own): capturable.  LF_MKD_ERR_BAD_ARG before any device is
 * touched (message "edge_layout_device: ...", through lf_mkd_last_error(NULL) when h is NULL): a null handle; with
 * n_edges > 0 a null pointer; an offset array not 8-byte or d_edge_image not 4-byte aligned; n_rows_total above 2^31 - 1.
 *
 * lf_mkd_gather_edge_rows_device brings rows of any kind from a pool into the edge layout -- keypoints (row_bytes 20) for
 * the verifiers, q8 rows (128) or f32 rows (512) for a call that has no edges form.  For edge e let (lo, len) be the range
 * [edge_offsets[e], edge_offsets[e+1]) read against capacity_rows as a pair is read against a total, and (first, n) its
 * image's rows: dst row lo + r = src row first + r for r < min(n, len).  row_bytes is a multiple of 4 in [4, 512]; d_src and
 * d_dst are 4-byte aligned.  Rows of dst that belong to no edge are untouched; nothing at or beyond n_rows_total is read and
 * nothing at or beyond capacity_rows is written, whatever the arrays hold.  One launch, no scratch, capturable; n_edges == 0
 * is LF_MKD_OK.  LF_MKD_ERR_BAD_ARG before any device is touched (message "gather_edge_rows_device: ..."): a null handle; a
 * null pointer; a bad row_bytes; d_src or d_dst not 4-byte aligned; a total or a capacity above 2^31 - 1; more than
 * 2^31 - 1 workgroups (floor(capacity_rows / 64) + n_edges).
 *
 * lf_mkd_match_q8_edges_device decides every edge.  For edge e let A be image edge_a[e] of pool a (nA rows), B image
 * edge_b[e] of pool b (nB rows), and (loA, lenA) / (loB, lenB) the edge's ranges of the two layouts against ea_capacity /
 * eb_capacity.
 *   a -> b      for r < min(nA, lenA) the entries loA + r of d_match_ab, d_best and d_second EQUAL what
 *               lf_mkd_match_q8_device(A, B) writes for row r without exclusion ranges: exact int32 sums, ties to the highest
 *               index, second == best when the maximum occurs twice, accepted iff ratio <= 0 || (float)best * ratio >
 *               (float)second; match values are local to B.  B is always the WHOLE image, whatever the b-side layout holds.
 *               With nB < 2 the outputs are -1 and INT32_MIN, the pairs call's rule.
 *   b -> a      when d_match_ba is given this direction is decided in the same launch, likewise over the whole A, for
 *               r < min(nB, lenB) at loB + r, with nA < 2 as the refusal.
 *   mutual      LF_MKD_MATCH_MUTUAL is lf_mkd_match_pairs_device's filter, unchanged, on (d_edge_offsets_a, ea_capacity,
 *               d_edge_offsets_b, eb_capacity).
 * d_edge_offsets_b, eb_capacity and d_match_ba may be NULL / 0 together unless the flag is set; d_best and d_second may be
 * NULL.  d_a and d_b must be 16-byte aligned.
 * Capacities and the grid: ea_capacity / eb_capacity are the sizes of the caller's output arrays, upper bounds of the
 * layouts' last entries (a caller who keeps counts on the device passes n_edges x its per-image cap).  The host sizes the
 * grid from them and never reads a device array; the grid is exactly what lf_mkd_match_q8_pairs_plan(ea_capacity,
 * eb_capacity, n_edges, d_match_ba != NULL) reports -- the same R, the same slot map, over the edge offsets.
 * Bounds, whatever the arrays hold: no row at or beyond a pool's total is read, no entry at or beyond a capacity is written,
 * entries of no edge are untouched.  The result of an edge depends on its two images, `ratio` and nothing else: not on
 * n_edges, not on the other edges, not on the run, not on the device's CU count.
 * Cost: as the pairs call, every workgroup streams its edge's whole other image through LDS; an image on k edges is read k
 * times from memory (L2 permitting) and copied nowhere.
 * One launch (three with LF_MKD_MATCH_MUTUAL), no scratch, no allocation, no host synchronisation, asynchronous on `stream`
 * (NULL: the handle's own): capturable in a hipGraph.  n_edges == 0 is LF_MKD_OK and writes nothing.
 * lf_mkd_match_overflowed is not affected.
 * LF_MKD_ERR_BAD_ARG, reported before any device is touched (the message starts with "match_q8_edges_device: " and is
 * reachable through lf_mkd_last_error(NULL) when h is NULL): a null handle; null d_a, d_b, image offsets or d_match_ab; a null
 * edge or layout array (d_edge_offsets_b only when d_match_ba is given); LF_MKD_MATCH_MUTUAL without d_match_ba; unknown flag
 * bits; d_a or d_b not 16-byte aligned; a total or a capacity above 2^31 - 1; a grid above 2^31 - 1 workgroups. */
int lf_mkd_edge_layout_device(lf_mkd *h, const uint64_t *d_image_offsets, uint32_t n_images, uint64_t n_rows_total,
                              const uint32_t *d_edge_image, uint32_t n_edges, uint64_t *d_edge_offsets, void *stream);
int lf_mkd_gather_edge_rows_device(lf_mkd *h, const void *d_src, uint32_t row_bytes, const uint64_t *d_image_offsets,
                                   uint32_t n_images, uint64_t n_rows_total, const uint32_t *d_edge_image,
                                   const uint64_t *d_edge_offsets, uint64_t capacity_rows, uint32_t n_edges, void *d_dst,
                                   void *stream);
int lf_mkd_match_q8_edges_device(lf_mkd *h, const uint8_t *d_a, const uint64_t *d_image_offsets_a, uint32_t n_images_a,
                                 uint64_t na_total, const uint8_t *d_b, const uint64_t *d_image_offsets_b, uint32_t n_images_b,
                                 uint64_t nb_total, const uint32_t *d_edge_a, const uint32_t *d_edge_b,
                                 const uint64_t *d_edge_offsets_a, uint64_t ea_capacity, const uint64_t *d_edge_offsets_b,
                                 uint64_t eb_capacity, uint32_t n_edges, float ratio, uint32_t flags, int32_t *d_match_ab,
                                 int32_t *d_match_ba, int32_t *d_best, int32_t *d_second, void *stream);
/* lf_mkd_build_tracks_device turns an edge list's matches into TRACKS: the sets of keypoints across the images of ONE pool
 * that the pairwise matches tie together -- what structure from motion, triangulation, map merging and loop closure consume.
 * One label per pool row, and per track its length and its number of conflicting rows.  There is one pool: both ids of an edge
 * index d_image_offsets.
 *   links       for edge e let (lo, len) be its range of d_edge_offsets_a read against ea_capacity as a pair is read against a
 *               total, and (firstA, nA) / (firstB, nB) the rows of images d_edge_a[e] / d_edge_b[e] against n_rows_total; an
 *               id at or beyond n_images names an empty image.  For r < min(nA, len) let j = d_match[lo + r]: entry lo + r is a
 *               LINK between pool rows firstA + r and firstB + j iff 0 <= j < nB; -1, any other negative value and any
 *               j >= nB are no link.  That is the convention of lf_mkd_match_q8_edges_device's d_match_ab, of the mutual
 *               filter's output and of both verifiers' `verified`: any of them is passed as it is.  Self edges, repeated
 *               edges, (j, i) beside (i, j) and layouts not made from these ids are ordinary input.
 *   d_track     int32 [n_rows_total].  Without LF_MKD_TRACKS_ACCUMULATE every entry r is written: the smallest pool row of
 *               r's connected component under the links.  A row on no link, or of no image, is its own track.  The label is a
 *               property of the component alone: it does not depend on the order of the edges, on n_edges beyond the link
 *               set, on the run or on the device's CU count.
 *   LF_MKD_TRACKS_ACCUMULATE   d_track is not initialised: it is read as the forest an earlier call left and the new links
 *               are added to it.  An entry p at index r with p < 0 || p > r is read as r, so parent <= index holds whatever
 *               the array holds, every walk ends, and a root is the minimum of its tree.  Links given in several calls, in any
 *               split and order, yield == the labels of one call with all of them: this is how a second match array (the
 *               guided matches beside the verified ones) or a later batch of edges is added.
 *   d_track_len optional, uint32 [n_rows_total]: at a label t the number of rows r with d_track[r] == t, 0 everywhere else.
 *   d_track_dup optional, uint32 [n_rows_total]: at a label t the sum over images m of max(c(m, t) - 1, 0), c(m, t) = the rows
 *               of image m (its range read as above) with label t; 0 everywhere else.  dup == 0: at most one keypoint per
 *               image, a consistent track.  Both statistics describe the whole forest after this call, accumulated links
 *               included.  The grid of this statistic is the slot map of d_image_offsets (floor(n_rows_total /
 *               LF_MKD_TRACKS_DUP_TILE) + n_images workgroups of LF_MKD_TRACKS_DUP_TILE rows), which serves every image when
 *               the offsets, read against the total, do not decrease -- an inverted range between two ordered neighbours
 *               included; its cost is quadratic in ONE image's row count (a row is compared with the labels of its image's rows
 *               in front of it), which is nothing at the 500 .. 8000 rows an image has here.  A row whose track has length 1
 *               skips that scan when d_track_len is given; without it every row scans (no scratch to keep the lengths in).
 * How: a lock-free union-find whose forest lives in d_track itself; a link hangs the larger of two roots under the smaller
 * with one compare-and-swap, so a root is the minimum of its tree (csrc/mkd_tracks.hip).  No workgroup waits for another.
 * Integer atomics only: exact and deterministic.
 * Launches: init (not with the flag), link (floor(ea_capacity / 256) + n_edges workgroups, only with n_edges > 0), flatten;
 * with a statistic a zeroing launch, one for d_track_len and one for d_track_dup -- a fixed number, sized by the host from
 * n_rows_total, ea_capacity, n_edges and n_images only; no device array is ever read by the host.  No scratch, no allocation,
 * no host synchronisation, asynchronous on `stream` (NULL: the handle's own): capturable in a hipGraph.  n_edges == 0 still
 * initialises, labels (every row its own track) and writes the statistics; n_rows_total == 0 is LF_MKD_OK and writes
 * nothing.  Whatever the arrays hold, nothing at or beyond n_rows_total or ea_capacity is read or written.
 * LF_MKD_ERR_BAD_ARG, reported before any device is touched (the message starts with "build_tracks_device: " and is
 * reachable through lf_mkd_last_error(NULL) when h is NULL): a null handle; null d_image_offsets or d_track; with
 * n_edges > 0 a null edge, layout or match array; an offset array not 8-byte or any other array not 4-byte aligned; unknown
 * flag bits; n_rows_total or ea_capacity above 2^31 - 1; a grid above 2^31 - 1 workgroups (d_track_dup's only when it is
 * given). */
int lf_mkd_build_tracks_device(lf_mkd *h, const uint64_t *d_image_offsets, uint32_t n_images, uint64_t n_rows_total,
                               const uint32_t *d_edge_a, const uint32_t *d_edge_b, const uint64_t *d_edge_offsets_a,
                               uint64_t ea_capacity, uint32_t n_edges, const int32_t *d_match, uint32_t flags,
                               int32_t *d_track, uint32_t *d_track_len, uint32_t *d_track_dup, void *stream);
#define LF_MKD_TRACKS_ACCUMULATE 1u /* flags: d_track holds an earlier call's forest; add the links to it */
#define LF_MKD_TRACKS_DUP_TILE (256) /* rows one workgroup of d_track_dup's launch owns (a build-time constant) */
/* lf_mkd_track_table_device turns the arrays lf_mkd_build_tracks_device leaves into a TRACK TABLE: per track the list of its
 * observations, as a CSR table, short and inconsistent tracks filtered out -- the form structure from motion, triangulation,
 * bundle adjustment and loop closure read.  N = n_rows_total; d_track, d_track_len, d_track_dup are [N] as that call wrote
 * them.
 *   reading     a label t is a ROOT iff 0 <= t < N and d_track[t] == t; a root is SELECTED iff d_track_len[t] >= min_len and,
 *               under LF_MKD_TRACK_TABLE_CONSISTENT, d_track_dup[t] == 0; row r is a MEMBER of selected t iff d_track[r] == t;
 *               a d_track[r] outside [0, N) makes r a member of nothing.
 *   order       the selected labels in ascending order are t_0 < t_1 < ... (the order of each track's smallest row); W_i is
 *               the 64-bit sum of d_track_len[t_j] over j < i.  Track i is KEPT iff i < track_capacity and
 *               W_{i+1} <= obs_capacity.  W does not decrease, so the kept tracks are a prefix 0 .. T - 1 and a track is never
 *               cut in the middle.  track_capacity >= floor(N / min_len) and obs_capacity >= N always suffice.
 *   d_counts    uint32 [4] = {T, O = W_T, the number of selected tracks, min(W of all selected tracks, 2^32 - 1)}; elements
 *               2 and 3 tell a caller that a capacity cut something.
 *   d_track_offsets   uint64, exactly track_capacity + 1 entries written: W_i for i <= T, O for T < i <= track_capacity -- a
 *               layout of track_capacity tracks whose tail is empty.
 *   d_obs_row   int32 [obs_capacity]: d_obs_row[W_i + k] = the k-th smallest member row of track i; entries at or beyond O
 *               are untouched.  May be NULL iff obs_capacity == 0.
 *   d_obs_image optional, uint32 [obs_capacity]: at the same positions the image m whose range of d_image_offsets, read
 *               against N exactly as lf_mkd_build_tracks_device reads it, holds the row, or 0xFFFFFFFF; specified for
 *               offsets that do not decrease.  d_image_offsets may be NULL iff d_obs_image is.
 *   d_row_track optional, int32 [N], every entry written: the table index of the row's track, or -1.
 * For arrays as lf_mkd_build_tracks_device leaves them a track's member count equals its d_track_len and all of the above
 * holds with ==.  For other contents the outputs other than d_counts are unspecified; even then the call ends, d_counts[0] <=
 * track_capacity, and nothing at or beyond N, track_capacity + 1 or obs_capacity is read or written.  N == 0 writes
 * d_counts = 0 and the offsets 0 and is LF_MKD_OK (the [N] arrays may then be NULL).
 * How (csrc/mkd_track_table.hip): a select-and-scan over the rows (two exact integer prefix sums), one key per row (the table
 * index of its label; rows of no kept track get a key above every index), and a stable LSD radix sort of (key, row) over the
 * bits of floor(N / min_len) only.  No atomic decides a position, no workgroup waits for another, integer arithmetic only:
 * the table is exact and does not depend on the run or on the CU count, and the cost does not depend on how the rows are
 * distributed over the tracks.
 * Launches: 4, then 3 per radix pass and 1 (none of these when lf_mkd_track_table_plan's passes or obs_capacity is 0); 1 for
 * N == 0 -- a fixed number, sized by the host from N, min_len and the capacities.  Asynchronous on `stream` (NULL: the
 * handle's own), no host synchronisation; no allocation once the handle's scratch has grown to the largest plan seen
 * (lf_mkd_track_table_plan's scratch_bytes), so a warmed-up call is capturable in a hipGraph.  The scratch belongs to the
 * handle: calls of one handle are stream-ordered.
 * LF_MKD_ERR_BAD_ARG, reported before any device is touched (the message starts with "track_table_device: " and is reachable
 * through lf_mkd_last_error(NULL) when h is NULL): a null handle or a null required array; min_len == 0;
 * LF_MKD_TRACK_TABLE_CONSISTENT without d_track_dup; d_obs_image without d_image_offsets; unknown flag bits; an offsets array
 * not 8-byte or any other array not 4-byte aligned; N or a capacity above 2^31 - 1. */
/* host only, no device, no handle: key_bits = the bits of floor(n_rows_total / min_len) (the bound on T the host knows), the
 * radix passes that cover them, the rows one workgroup sorts, and the scratch the device call grows the handle to (0 for
 * n_rows_total == 0); any output may be NULL.  LF_MKD_ERR_BAD_ARG ("track_table_plan: "): min_len == 0, n_rows_total above
 * 2^31 - 1. */
int lf_mkd_track_table_plan(uint64_t n_rows_total, uint32_t min_len, uint32_t *key_bits, uint32_t *passes, uint32_t *block_rows,
                            uint64_t *scratch_bytes);
int lf_mkd_track_table_device(lf_mkd *h, const uint64_t *d_image_offsets, uint32_t n_images, uint64_t n_rows_total,
                              const int32_t *d_track, const uint32_t *d_track_len, const uint32_t *d_track_dup, uint32_t min_len,
                              uint32_t flags, uint64_t track_capacity, uint64_t obs_capacity, uint64_t *d_track_offsets,
                              int32_t *d_obs_row, uint32_t *d_obs_image, int32_t *d_row_track, uint32_t *d_counts, void *stream);
#define LF_MKD_TRACK_TABLE_CONSISTENT (1u) /* flags: only tracks with d_track_dup[t] == 0 */
/* dst row k = src row d_obs_row[k] for k < min(d_counts[1], obs_capacity), rows of row_bytes bytes (keypoints: 20, q8 rows:
 * 128); an index outside [0, n_rows_total) writes a zero row, rows beyond the count are untouched.  One launch, its grid sized
 * from obs_capacity; the count is read on the device.  Asynchronous, no scratch, capturable.  LF_MKD_ERR_BAD_ARG
 * ("gather_track_rows_device: "): a null handle or array, row_bytes not a multiple of 4 within 4 .. 512, an array not 4-byte
 * aligned, n_rows_total or obs_capacity above 2^31 - 1. */
int lf_mkd_gather_track_rows_device(lf_mkd *h, const void *d_src, uint32_t row_bytes, uint64_t n_rows_total,
                                    const int32_t *d_obs_row, const uint32_t *d_counts, uint64_t obs_capacity, void *d_dst,
                                    void *stream);
/* lf_mkd_link_table_device turns an edge list's match array into a LINK TABLE: per edge the compact list of its
 * correspondences, as a CSR table, with the per-edge counts and a pruned copy of the match array -- the two-view result a pose
 * solver, a bundle adjuster and a two-view-geometry database read, and the place where an edge the geometry does not support
 * is dropped before lf_mkd_build_tracks_device takes its links.  There is one pool: both ids of an edge index d_image_offsets.
 * The inputs are read exactly as lf_mkd_build_tracks_device reads them; its rule, once more:
 *   links       for edge e let (lo, len) be its range of d_edge_offsets_a read against ea_capacity as a pair is read against a
 *               total, and (firstA, nA) / (firstB, nB) the rows of images d_edge_a[e] / d_edge_b[e] against n_rows_total; an
 *               id at or beyond n_images names an empty image.  For r < min(nA, len) let j = d_match[lo + r]: entry lo + r is a
 *               LINK between pool rows firstA + r and firstB + j iff 0 <= j < nB; -1, any other negative value and any
 *               j >= nB are no link.  L_e is the number of links of edge e.
 *   selection   edge e is SELECTED iff L_e >= min_links; min_links == 0 selects every edge.
 *   prefix, cut W_e is the 64-bit sum of L_f over the selected f < e.  Edge e is KEPT iff it is selected and
 *               W_{e+1} <= link_capacity.  W does not decrease, so no edge is cut in the middle and no kept edge follows a cut
 *               one.  O is the sum of L_e over the kept edges.  link_capacity >= ea_capacity always suffices.
 *   d_link_offsets   uint64, exactly n_edges + 1 entries written: min(W_e, O) -- an ordinary pair layout over the same edges, in
 *               which an edge that is not kept has an empty range; model[e] / stats[e] of the verifiers stay aligned with it.
 *   d_link_a, d_link_b   int32 [link_capacity]: at W_e + k the k-th link of kept edge e in ascending r, as the pool rows
 *               firstA + r and firstB + j; under LF_MKD_LINK_TABLE_LOCAL as r and j, the rows local to their images.  Entries
 *               at or beyond O are untouched.  Both may be NULL iff link_capacity == 0.
 *   d_link_edge optional, uint32 [link_capacity]: e at the same positions.
 *   d_edge_links optional, uint32 [n_edges]: L_e of every edge, selected or not.
 *   d_match_kept optional, int32, indexed like d_match: for every entry lo + r, r < min(nA, len), of every edge it holds
 *               d_match[lo + r] if the entry is a link of a KEPT edge and -1 otherwise; entries of no edge, and entries at or
 *               beyond ea_capacity, are untouched.  It may be d_match itself (in place: every entry is read before it is
 *               written, by the same thread).  Passed to lf_mkd_build_tracks_device it carries exactly the kept edges' links.
 *   d_counts    uint32 [4] = {the kept edges, O, the selected edges, min(W_{n_edges}, 2^32 - 1)}; elements 2 and 3 tell a
 *               caller what was wanted, so that a capacity that cut something shows.  Element 1 sits where
 *               lf_mkd_gather_track_rows_device reads its count: without LF_MKD_LINK_TABLE_LOCAL that call, given d_link_a (and
 *               once more d_link_b) as d_obs_row, this d_counts and link_capacity as obs_capacity, brings keypoints or any
 *               4 .. 512-byte rows into the table's order.  There is no other gather.
 * All of this is specified for layouts that do not decrease.  Whatever the arrays hold the call ends, d_counts[1] <=
 * link_capacity, and nothing is read or written at or beyond n_rows_total, ea_capacity, n_edges + 1 or link_capacity.
 * n_edges == 0 is LF_MKD_OK and writes d_counts = 0 and d_link_offsets[0] = 0.
 * How (csrc/mkd_link_table.hip): lf_mkd_build_tracks_device's slot map (one workgroup per slot of slot_entries entries of one
 * edge, so slot order is edge order, then row order); a count per slot (ballot and popcount) and per edge (an integer add: a
 * sum does not depend on its order), an exclusive 64-bit scan of the selected slots' counts over scan_levels levels of
 * fan-out scan_fanout, the cut per edge, and a scatter to the slot's prefix plus the rank within the slot.  No atomic decides
 * a position, no workgroup waits for another, integer arithmetic only: the table is exact and does not depend on the run or
 * on the CU count.
 * Launches, with L = lf_mkd_link_table_plan's scan_levels: 2 L + 4 (zero, count, L - 1 up the scan and L down, cut, scatter,
 * finalise); 2 L + 3 when link_capacity == 0 and d_match_kept is NULL (no scatter); 1 for n_edges == 0 -- a fixed number,
 * sized by the host from ea_capacity, n_edges and link_capacity only; no device array is ever read by the host.  Asynchronous
 * on `stream` (NULL: the handle's own), no host synchronisation; no allocation once the handle's scratch has grown to the
 * largest plan seen (lf_mkd_link_table_plan's scratch_bytes), so a warmed-up call is capturable in a hipGraph.  The scratch
 * belongs to the handle: calls of one handle are stream-ordered.
 * LF_MKD_ERR_BAD_ARG, reported before any device is touched (the message starts with "link_table_device: " and is reachable
 * through lf_mkd_last_error(NULL) when h is NULL): a null handle; null d_image_offsets, d_link_offsets or d_counts; with
 * n_edges > 0 a null edge, layout or match array; with link_capacity > 0 a null d_link_a or d_link_b; unknown flag bits; an
 * offset array not 8-byte or any other array not 4-byte aligned; n_rows_total, ea_capacity or link_capacity above 2^31 - 1; a
 * grid above 2^31 - 1 workgroups (floor(ea_capacity / slot_entries) + n_edges). */
/* host only, no device, no handle: what the device call will use, and the only place that knows it -- slot_entries = the
 * entries per slot, slots = floor(ea_capacity / slot_entries) + n_edges (the grid of the count and of the scatter),
 * scan_fanout = the slots one workgroup of the scan sums, scan_levels = the smallest L >= 1 with scan_fanout^L >= slots (0 for
 * n_edges == 0), scratch_bytes = the scratch the device call grows the handle to (0 for n_edges == 0; otherwise 20 bytes a
 * slot, 12 bytes a value of scan levels 1 .. L - 1, level k having ceil(slots / scan_fanout^k) values, 4 bytes an edge and
 * 16); any output may be NULL.  LF_MKD_ERR_BAD_ARG ("link_table_plan: "): ea_capacity above 2^31 - 1, slots above 2^31 - 1. */
int lf_mkd_link_table_plan(uint64_t ea_capacity, uint32_t n_edges, uint32_t *slot_entries, uint64_t *slots,
                           uint32_t *scan_fanout, uint32_t *scan_levels, uint64_t *scratch_bytes);
int lf_mkd_link_table_device(lf_mkd *h, const uint64_t *d_image_offsets, uint32_t n_images, uint64_t n_rows_total,
                             const uint32_t *d_edge_a, const uint32_t *d_edge_b, const uint64_t *d_edge_offsets_a,
                             uint64_t ea_capacity, uint32_t n_edges, const int32_t *d_match, uint32_t min_links,
                             uint32_t flags, uint64_t link_capacity, uint64_t *d_link_offsets, int32_t *d_link_a,
                             int32_t *d_link_b, uint32_t *d_link_edge, uint32_t *d_edge_links, int32_t *d_match_kept,
                             uint32_t *d_counts, void *stream);
#define LF_MKD_LINK_TABLE_LOCAL (1u)  /* d_link_a / d_link_b hold rows local to their images, not pool rows */
/* lf_mkd_select_edges_device turns a vote table into CANDIDATE EDGES: per image the k images that received the most votes from
 * it, and the edge list those picks make -- the step between lf_mkd_vote_groups_device and lf_mkd_edge_layout_device /
 * lf_mkd_match_q8_edges_device, which take d_edge_a / d_edge_b unchanged.  d_votes is [n_a][n_b] uint32, as
 * lf_mkd_vote_groups_device writes it.
 *   candidates  of row i: the columns j < n_b with votes[i][j] >= min_votes and, under LF_MKD_SELECT_SKIP_SELF, j != i.
 *               min_votes == 0 admits columns without a vote; a caller passes 1 to drop them.  Votes are compared as unsigned
 *               32-bit values; 2^32 - 1 is an ordinary value.
 *   order       larger votes first, among equal votes the LOWER column first: (-votes, j), the order a retrieval result is
 *               printed in, a stable numpy argsort of -votes (as int64) over the candidates.  This is NOT the rule of
 *               lf_mkd_knn_q8_device and of the matchers, which prefer the HIGHER index among equal scores.
 *   picks       P(i) = the first min(k, candidates) columns of that order.
 *   d_rank      optional, int32 [n_a][k]: P(i) in order, -1 in the slots behind it.
 *   d_rank_votes optional, uint32 [n_a][k]: the votes of those picks, 0 behind them.  Exactly n_a * k entries of each are
 *               written.  With n_a == 1 this is the retrieval answer for one query.
 *   edges       the picks are walked in the order i ascending, then rank ascending.  Without LF_MKD_SELECT_UNIQUE every pick
 *               (i, j) is the edge (i, j).  With it (one pool: n_a == n_b) a pick (i, j) is an edge iff j > i, or j < i and i is
 *               not in P(j); a self pick is never an edge; the edge is written as (min(i, j), max(i, j)).  So a pair that
 *               either image picked appears exactly once, at the position of the smaller image's pick if it made one, and
 *               the matcher behind does not match a mutual pick twice.  S is the number of edges, E = min(S, edge_capacity)
 *               the number kept: the first E.
 *   d_edge_a, d_edge_b   uint32 [edge_capacity], exactly edge_capacity entries of each written: the kept edges, then 0xFFFFFFFF
 *               in both, which names an empty image to every edge-list call -- a caller passes n_edges = edge_capacity
 *               downstream and never reads the count.  Both may be NULL iff edge_capacity == 0.  edge_capacity >= n_a * k
 *               always suffices.
 *   d_edge_votes optional, uint32 [edge_capacity]: votes[i][j] of the pick that made the edge, 0 in the padding.
 *   d_counts    uint32 [4] = {E, S, the number of picks, the number of rows with at least one pick}; element 1 tells a caller
 *               what was wanted, so that a capacity that cut something shows.
 * The result depends on the table, k, min_votes, flags and edge_capacity alone: not on the run, not on the CU count, not on
 * the form the plan chose.  Nothing is read or written at or beyond n_a * n_b, n_a * k or edge_capacity, whatever the table
 * holds.  n_a == 0 is LF_MKD_OK and writes d_counts = 0 and the padding.
 * How (csrc/mkd_select_edges.hip): every candidate is one 64-bit key, votes << 32 | (0xFFFFFFFF - j), so the order is a plain
 * unsigned maximum and keys are unique within a row.  The selection reads each row once, with 16-byte loads where its address
 * allows; a lane keeps its compiled_k largest keys in a sorted register list behind a ballot gate (lf_mkd_knn_q8_device's
 * pattern), and lanes, waves and -- where there are too few rows to fill the device and a row is cut into segments -- segments
 * are merged by maxima of keys, which is exact and independent of the order of arrival.  Rows of at most 2048 columns take one
 * wave each, four to a workgroup; longer ones a workgroup per row or segment.  Then one thread per pick slot decides whether
 * it is an edge (under LF_MKD_SELECT_UNIQUE by k reads of the rank table, which lives in the scratch when d_rank is NULL), an
 * exact integer exclusive scan gives every edge its position, and a scatter writes edges and padding.  No atomic at all, no
 * workgroup waits for another, integer arithmetic only.
 * Launches (lf_mkd_select_edges_plan's `launches`): 4 -- select, flag, scan, scatter --, 5 when rows are cut into segments
 * (the merge), 1 for n_a == 0: a fixed number, sized by the host from the scalar arguments only; no device array is ever read
 * by the host.  Asynchronous on `stream` (NULL: the handle's own), no host synchronisation; no allocation once the handle's
 * scratch has grown to the largest plan seen (the plan's scratch_bytes), so a warmed-up call is capturable in a hipGraph.  The
 * scratch belongs to the handle: calls of one handle are stream-ordered.
 * LF_MKD_ERR_BAD_ARG, reported before any device is touched (the message starts with "select_edges_device: " and is reachable
 * through lf_mkd_last_error(NULL) when h is NULL): a null handle; a null d_votes with n_a > 0; a null d_counts; with
 * edge_capacity > 0 a null d_edge_a or d_edge_b; n_b == 0 with n_a > 0; k == 0 or above LF_MKD_SELECT_MAX_K; unknown flag
 * bits; LF_MKD_SELECT_UNIQUE with n_a != n_b; an array not 4-byte aligned; n_a * n_b (lf_mkd_vote_groups_device's limit),
 * n_a * k or edge_capacity above 2^31 - 1. */
/* host only, no device, no handle: what the device call will use, and the only place that knows it -- compiled_k = the
 * instantiation that serves k (4, 8, 16 or 32), rows_per_workgroup = 4 (one wave per row) or 1, workgroups = the grid of the
 * selection (ceil(n_a / 4); n_a times the segments of a row otherwise; 0 for n_a == 0), launches and scratch_bytes = what the
 * device call does and grows the handle to (12 bytes a pick slot, 16 bytes per 256 slots, 8 bytes a key of every segment when
 * rows are cut; 0 for n_a == 0); any output may be NULL.  LF_MKD_ERR_BAD_ARG ("select_edges_plan: "): the device call's
 * refusals that concern n_a, n_b, k, edge_capacity and flags. */
int lf_mkd_select_edges_plan(uint32_t n_a, uint32_t n_b, uint32_t k, uint64_t edge_capacity, uint32_t flags,
                             uint32_t *compiled_k, uint32_t *rows_per_workgroup, uint64_t *workgroups, uint32_t *launches,
                             uint64_t *scratch_bytes);
int lf_mkd_select_edges_device(lf_mkd *h, const uint32_t *d_votes, uint32_t n_a, uint32_t n_b, uint32_t k, uint32_t min_votes,
                               uint32_t flags, uint64_t edge_capacity, int32_t *d_rank, uint32_t *d_rank_votes,
                               uint32_t *d_edge_a, uint32_t *d_edge_b, uint32_t *d_edge_votes, uint32_t *d_counts,
                               void *stream);
#define LF_MKD_SELECT_SKIP_SELF (1u)  /* column i is no candidate of row i */
#define LF_MKD_SELECT_UNIQUE (2u)     /* one pool (n_a == n_b): every unordered pair at most once, as (smaller, larger) */
#define LF_MKD_SELECT_MAX_K (32)
/* lf_mkd_covisibility_device turns a track table into the COVISIBILITY TABLE: per pair of images, how many tracks they share --
 * what structure from motion, keyframe graphs, local bundle-adjustment windows and next-best-view choice read first, and, with
 * the pairs already matched zeroed, the [images][images] table lf_mkd_select_edges_device takes as it is for a second round
 * of candidate edges.  Inputs are a table as lf_mkd_track_table_device leaves it: d_track_offsets (uint64, track_capacity + 1
 * entries), d_obs_image (uint32, obs_capacity entries) and that call's d_counts as d_table_counts.
 *   reading     T = min(d_table_counts[0], track_capacity), O = min(d_table_counts[1], obs_capacity).  Track t < T is the range
 *               [lo, hi) of d_track_offsets[t], d_track_offsets[t + 1], each read against O as a pair is read against a total:
 *               beyond O is O, an inverted range is empty.
 *   counted     position k of track t is COUNTED iff (k == lo or d_obs_image[k] != d_obs_image[k - 1]) and d_obs_image[k] <
 *               n_images.  The comparison with k - 1 is with the raw entry, before the range test; 0xFFFFFFFF and any other id
 *               at or beyond n_images is never counted.  A table made over image offsets that do not decrease lists a
 *               track's images in non-decreasing order, and the rule is then "one count per distinct image of the track",
 *               inconsistent tracks included; for any other contents the rule is still exactly this rule.
 *   table       C[i][j], i != j: the number of ordered pairs (p, q) of distinct counted positions of one track with images i
 *               and j, summed over the tracks; C[i][i]: the number of counted positions with image i.  For such tables:
 *               C[i][j] = the tracks seen in both i and j, C[i][i] = the tracks seen in i, C symmetric.
 *   d_covis     uint32 [n_images][n_images]; exactly n_images^2 entries are written: C mod 2^32.  Under
 *               LF_MKD_COVIS_ACCUMULATE the table is not zeroed and C is added to what it holds, mod 2^32: the tracks of one
 *               table given in several calls, in any split, yield == one call with all of them.
 *   mask        d_edge_a / d_edge_b, uint32 [n_edges], optional (both NULL iff n_edges == 0): after the counting, for every
 *               e < n_edges with both ids < n_images, d_covis[a][b] and d_covis[b][a] are set to 0; other entries are
 *               skipped, so lf_mkd_select_edges_device's padded lists pass whole.  Self edges, repeated edges and (j, i)
 *               beside (i, j) are ordinary input.  Under LF_MKD_COVIS_ACCUMULATE the mask applies to the sum.
 * For offsets that do not decrease (after the clamp to O) all of this holds with ==, whatever d_obs_image holds.  For other
 * offsets d_covis is unspecified; the call still ends, and nothing is read or written at or beyond track_capacity + 1,
 * obs_capacity, n_edges or n_images^2.  n_images == 0 is LF_MKD_OK and writes nothing; T == 0 still zeroes and masks.
 * How (csrc/mkd_covisibility.hip): a group of `form` lanes (4 .. 64) holds a track's positions one per lane, a chunk at a time;
 * the counted lanes of one chunk are visited through the set bits of a ballot, their image is broadcast by a lane permute and
 * every counted lane of the other chunk adds one pair, so a track of L distinct images costs L ceil(L / form) steps of full
 * lanes for its L^2 adds.  Tracks of more than 16 form positions are marked in a bitmap of the observation array (the scratch)
 * and taken by a second launch, a wave per 64 marked positions against the whole track.  COST BOUND: only counted positions
 * cost a step, so one track of L positions with D distinct images -- a table made without LF_MKD_TRACK_TABLE_CONSISTENT can
 * hold one track of every row -- costs at most D ceil(L / 64) steps and D ceil(L / 64) loads of 64 positions: (distinct
 * images) x (track length), never length squared.  Integer atomic adds only, so the table is exact and independent of the run,
 * the CU count and the form; with at most 64 images a workgroup counts into a private table in LDS and adds it once
 * (LF_MKD_COVIS_FORM_LDS in the plan's form).  No workgroup waits for another.
 * Launches (lf_mkd_covisibility_plan's `launches`): zero (a kernel, not a memset node, see lf_mkd_vote_groups_device; under
 * LF_MKD_COVIS_ACCUMULATE it zeroes the bitmap alone), the two counting launches (none when a capacity is 0), the mask
 * (n_edges > 0): 1 to 4, none for n_images == 0 -- a fixed number, sized by the host from the scalar arguments only; no device
 * array is ever read by the host.  Asynchronous on `stream` (NULL: the handle's own), no host synchronisation; no allocation
 * once the handle's scratch has grown to the largest plan seen (4 bytes per 2048 observations), so a warmed-up call is
 * capturable in a hipGraph.  The scratch belongs to the handle: calls of one handle are stream-ordered.
 * LF_MKD_ERR_BAD_ARG, reported before any device is touched (the message starts with "covisibility_device: " and is reachable
 * through lf_mkd_last_error(NULL) when h is NULL): a null handle; a null d_covis with n_images > 0; a null d_table_counts; a
 * null d_track_offsets; a null d_obs_image with obs_capacity > 0; only one of the edge arrays, or n_edges > 0 without them;
 * unknown flag bits; offsets not 8-byte aligned or another array not 4-byte aligned; n_images^2 above 2^31 - 1
 * (lf_mkd_vote_groups_device's limit); track_capacity or obs_capacity above 2^31 - 1. */
/* host only, no device, no handle: what the device call will do, and the only place that knows it -- form = the lanes that
 * share a track (4, 8, 16, 32, 64: the smallest that holds twice the mean track length the capacities allow, never more than
 * the images), plus LF_MKD_COVIS_FORM_LDS iff workgroups count in LDS first; workgroups = the grid of the first counting
 * launch (with LF_MKD_COVIS_FORM_LDS at most 2^22 / n_images^2, or 256: every workgroup adds its table at its end); launches and scratch_bytes = what the device call does and grows the handle to; all 0 for n_images == 0; any output
 * may be NULL.  LF_MKD_ERR_BAD_ARG ("covisibility_plan: "): the device call's refusals that concern the scalars. */
int lf_mkd_covisibility_plan(uint32_t n_images, uint64_t track_capacity, uint64_t obs_capacity, uint64_t n_edges, uint32_t flags,
                             uint32_t *form, uint64_t *workgroups, uint32_t *launches, uint64_t *scratch_bytes);
int lf_mkd_covisibility_device(lf_mkd *h, const uint64_t *d_track_offsets, uint64_t track_capacity, const uint32_t *d_obs_image,
                               uint64_t obs_capacity, const uint32_t *d_table_counts, uint32_t n_images, const uint32_t *d_edge_a,
                               const uint32_t *d_edge_b, uint64_t n_edges, uint32_t flags, uint32_t *d_covis, void *stream);
#define LF_MKD_COVIS_ACCUMULATE (1u)  /* flags: d_covis is not zeroed, the table is added to what it holds */
#define LF_MKD_COVIS_FORM_LDS (256u)  /* in the plan's form: a workgroup counts into a private table in LDS first */
/* lf_mkd_two_view_pose_device turns every verified edge of a calibrated collection into a RELATIVE POSE: the rotation R and
 * the unit translation t of camera b relative to camera a (x_b = R x_a + t), chosen among the four candidates of the edge's
 * essential matrix by a vote of the edge's links, with the links' triangulated points -- what structure from motion reads to
 * pick its initial pair (many links with real parallax), to reject an edge whose F is no essential matrix under the
 * intrinsics, and to seed points.  Inputs are what the calls above leave on the device: d_F [n_edges][9] of
 * lf_mkd_verify_fundamental_device (b^T F a = 0, pixels), the link table d_link_offsets / d_link_a / d_link_b of
 * lf_mkd_link_table_device WITHOUT LF_MKD_LINK_TABLE_LOCAL (pool rows), the pool's keypoints (only x and y are read), the edge
 * list, and d_intrinsics [n_images][4] = fx, fy, cx, cy per image.
 *   reading     edge e's links are the range of d_link_offsets[e], d_link_offsets[e + 1] read against link_capacity as a pair
 *               is read against a total: an offset beyond it is link_capacity, an inverted range is empty.  Entry k of the
 *               range is a LINK iff 0 <= d_link_a[k] < n_rows_total and 0 <= d_link_b[k] < n_rows_total; any other entry is
 *               no link: it counts nowhere and its point is the "none" row.
 * Outputs per edge e:
 *   d_R         f32 [n_edges][9], row-major; d_t f32 [n_edges][3], |t| = 1.
 *   d_stats     uint32 [n_edges][4] = {links in front of both cameras under the chosen pose, the largest such count among the
 *               other three candidates, the chosen candidate c in 0 .. 3 (0xFFFFFFFF: none), in-front links whose parallax
 *               angle is at least min_parallax_deg}.
 *   d_sigma     optional, f32 [n_edges][3]: E's singular values over the largest, {1, s2/s1, s3/s1}.  A true essential matrix
 *               gives {1, 1, 0}; wrong intrinsics or a wrong F show here.
 *   d_points    optional, f32 [link_capacity][4]: per link, at its position in the table, {X, Y, Z in camera a's frame at
 *               |t| = 1, the COSINE of the parallax angle}; {0, 0, 0, 2} (the "none" row) for an entry that is no link or not
 *               in front under the chosen pose.  Entries outside every edge's range are untouched.
 * The algorithm, exactly (the kernel's own arithmetic, csrc/mkd_pose_math.h, built for the host, reproduces every output bit:
 * tests/cpp/pose_twin.cpp; a float64 numpy restatement: tests/pose_cases.py).  Only correctly rounded f64 operations are used
 * (+ - * /, sqrt) in a fixed order without contraction, with fixed iteration counts and no transcendental on the device:
 * cos(min_parallax_deg) is formed once on the host in double (cmin), and every point output is a cosine, not an angle.
 *   1. E = Kb^T F Ka in f64 from the f32 inputs: M = F Ka row by row (f0 fx, f1 fy, f0 cx + f1 cy + f2), then fxb M_0,
 *      fyb M_1, cxb M_0 + cyb M_1 + M_2, every sum left to right.
 *   2. SVD: S = E^T E (each entry a sum of three products, left to right), eigen-decomposed by 6 sweeps of cyclic Jacobi in
 *      f64, the F refit's rotation (pairs (0,1) (0,2) (1,2); theta = (s_qq - s_pp) / (2 s_pq), t = sign(theta) / (|theta| +
 *      sqrt(theta^2 + 1)), c = 1 / sqrt(t^2 + 1), s = t c; none where s_pq = 0).  Eigenvalues w are sorted descending, the lower
 *      index first on a tie; s_i = sqrt(max(w_i, 0)).  u1 = E v1 / |E v1|; u2 = E v2 - (u1 . E v2) u1, normalised;
 *      u3 = u1 x u2, v3 = v1 x v2 (both determinants +1).  With W = [[0,-1,0],[1,0,0],[0,0,1]]: R1 = U W V^T =
 *      (u2 v1^T - u1 v2^T) + u3 v3^T, R2 = U W^T V^T = (u1 v2^T - u2 v1^T) + u3 v3^T.  Candidates c = 0: (R1, +u3), 1: (R1, -u3),
 *      2: (R2, +u3), 3: (R2, -u3).  Eigenvector signs are the Jacobi's own: another SVD may number the candidates differently.
 *   3. Vote: for a link, xa = ((x - cx) / fx, (y - cy) / fy, 1) from its a row under image a's intrinsics, xb likewise, in
 *      f64; p = R xa, q = xb; det = (p.p)(q.q) - (p.q)^2, na = (p.q)(q.t) - (p.t)(q.q), nb = (p.p)(q.t) - (p.q)(p.t).  The link is
 *      IN FRONT iff det > 0 and na > 0 and nb > 0 (the two depths' signs; no division decides anything).  It has PARALLAX iff it
 *      is in front and p.q <= cmin sqrt((p.p)(q.q)).  NaN coordinates need no rule: every comparison is false.
 *   4. Choice: the candidate with the largest in-front count, the lowest c on a tie.
 *   5. Points: la = na / det, lb = nb / det, X = (la xa + R^T (lb xb - t)) / 2 (the midpoint of the two rays' closest points,
 *      in camera a's frame), the cosine (p.q) / sqrt((p.p)(q.q)); rounded to f32 at the store, as R, t and sigma are.
 *   6. No pose: R, t and sigma all zero, stats {0, 0, 0xFFFFFFFF, 0}, every entry of the edge's range the "none" row; the status
 *      stays LF_MKD_OK.  That is the outcome iff an image id is at or beyond n_images (lf_mkd_select_edges_device's 0xFFFFFFFF
 *      padding passes whole), an intrinsic is not finite or fx or fy is <= 0, a value of F is not finite or F is all zero, s1
 *      is not finite and positive or s2 <= 1e-3 s1 (a rank-1 F), or the best count is 0.
 * Counts are integer sums: every output bit depends on the edge's own inputs alone, not on the other edges of the call, the
 * run, the CU count or the kernel's form; edge e of a batched call equals a single-edge call, a captured call replays to the
 * same bits.  Whatever the arrays hold the call ends and nothing is read or written at or beyond n_rows_total, n_images,
 * n_edges (+ 1 for the offsets) or link_capacity.  n_edges == 0 is LF_MKD_OK and writes nothing.
 * How (csrc/mkd_two_view_pose.hip): ONE launch, one workgroup of 256 threads per edge; thread 0 decomposes E into LDS, the
 * workgroup walks the links 256 at a time and counts the four candidates by ballot and popcount, chooses, and walks them once
 * more for the points and the parallax count.  No scratch, no allocation, no atomic, nobody waits; asynchronous on `stream`
 * (NULL: the handle's own), no host synchronisation, capturable in a hipGraph.
 * LF_MKD_ERR_BAD_ARG, reported before any device is touched (the message starts with "two_view_pose_device: " and is reachable
 * through lf_mkd_last_error(NULL) when h is NULL): a null handle; with n_edges > 0 a null edge array, d_F, d_link_offsets, d_R,
 * d_t or d_stats, a null d_intrinsics with n_images > 0, a null d_link_a or d_link_b with link_capacity > 0, a null d_kps with
 * link_capacity > 0 and n_rows_total > 0; flags other than 0 (none is defined); min_parallax_deg outside [0, 180] or NaN;
 * d_link_offsets not 8-byte or any other array not 4-byte aligned; n_rows_total, link_capacity or n_edges above 2^31 - 1. */
int lf_mkd_two_view_pose_device(lf_mkd *h, const lf_mkd_keypoint *d_kps, uint64_t n_rows_total, const uint32_t *d_edge_a,
                                const uint32_t *d_edge_b, uint32_t n_edges, const float *d_intrinsics, uint32_t n_images,
                                const float *d_F, const uint64_t *d_link_offsets, const int32_t *d_link_a, const int32_t *d_link_b,
                                uint64_t link_capacity, float min_parallax_deg, uint32_t flags, float *d_R, float *d_t,
                                uint32_t *d_stats, float *d_sigma, float *d_points, void *stream);
/* Host pointers, ONE pair, synchronous: F [9], Ka [4] and Kb [4] (fx, fy, cx, cy), the two images' keypoints and a match array
 * [na] read by the verifiers' rule (row i of a and row match[i] of b are a link iff 0 <= match[i] < nb; pass the verifier's
 * `verified`).  The links are built on the host and go through the device call; R [9], t [3], stats [4], optional sigma [3]
 * and optional points [na][4], indexed like a (the "none" row where row i has no link).  LF_MKD_ERR_BAD_ARG ("two_view_pose: "):
 * a null handle or required pointer, flags other than 0, min_parallax_deg outside [0, 180] or NaN, na + nb above 2^31 - 1. */
int lf_mkd_two_view_pose(lf_mkd *h, const float *F, const float *Ka, const float *Kb, const lf_mkd_keypoint *kps_a, uint64_t na,
                         const lf_mkd_keypoint *kps_b, uint64_t nb, const int32_t *match, float min_parallax_deg, uint32_t flags,
                         float *R, float *t, uint32_t *stats, float *sigma, float *points);

/* lf_mkd_triangulate_tracks_device gives every track of a track table its 3-D POINT under known camera poses: what
 * incremental structure from motion builds after its initial pair, what a triangulator over poses from odometry or a rig
 * builds, what seeds bundle adjustment.  ONE launch, nothing read back.
 * Reads: the track table as lf_mkd_track_table_device leaves it, read exactly as lf_mkd_covisibility_device reads it (T =
 * min(d_table_counts[0], track_capacity) tracks, O = min(d_table_counts[1], obs_capacity) positions, track t = positions
 * [d_track_offsets[t], d_track_offsets[t + 1]) with both ends clamped to O, an inverted range empty); the pool keypoints (x and
 * y alone); d_intrinsics [n_images][4] = fx, fy, cx, cy as in the pose call; d_poses [n_images][12] = R row-major, then t,
 * WORLD TO CAMERA: x_cam = R X + t (lf_mkd_two_view_pose_device's convention with camera a's frame as the world: a = [I | 0],
 * b = [R | t]).  R is used as given; its orthonormality is the caller's business.
 * A position k of a track is USABLE iff 0 <= d_obs_row[k] < n_rows_total, d_obs_image[k] < n_images, that image's intrinsics
 * are finite with fx, fy > 0, its 12 pose values are finite and R is not all zero, and the keypoint's x and y are finite.  An
 * all-zero R is the pose call's "no pose": it says "this image is not registered yet", so a partial pose array passes as it is.
 * The algorithm, exactly (f64, + - * / and sqrt alone, contraction off, the order csrc/mkd_triangulate_math.h fixes;
 * thr2 = max_reproj_px^2, formed once on the host in double):
 *   1. A usable position contributes nine values: with xn = ((x - cx) / fx, (y - cy) / fy, 1), d = R^T xn, u = d / sqrt(d.d)
 *      and c = 0 - R^T t, the six distinct entries of P = I - u u^T and the three of P c = c - u (u.c).
 *   2. The CANONICAL SUM over a set S of positions has 4 slots: slot j sums, from +0.0 and in ascending position, the
 *      contributions of the positions of S with (position within the track) mod 4 == j; the slots are then combined as
 *      (s0 + s2) + (s1 + s3).  This order is the contract: it lets 4 lanes own a track and still equal a serial twin bit
 *      for bit, whatever the launch shape, the track's place in the call or the CU count.  (4, not 8: tracks are 3 to 4
 *      long on average, and 8 lanes per track took 1.9 x as long on a table of pairs; profiles/triangulate.md.)
 *   3. Solve A X = b (A symmetric 3x3 from the first six sums, b the last three) by cofactors, X = adj(A) b / det.  SINGULAR
 *      iff not (det > 1e-12 m^3), m = (a00 + a11 + a22) / 3: a guard against exactly degenerate rays (for two rays det =
 *      2 sin^2 of their angle, so it trips below about 1e-6 rad), not a quality gate -- the parallax output is.
 *   4. A usable position is an INLIER of X iff, with p = R X + t (each row summed left to right), p_z > 0 and ex^2 + ey^2 <=
 *      thr2, ex = fx (p_x / p_z) + cx - x, ey likewise.  A NaN fails every comparison.
 *   5. PAIR HYPOTHESES: the candidates are the first min(U, 8) usable positions in ascending order (U = the usable
 *      positions of the track), the hypotheses the pairs (ci, cj), ci < cj, of candidate indices in lexicographic order; each
 *      is step 3 over the canonical sum of its two positions, scored by its inliers among ALL usable positions.  A singular
 *      pair is skipped; the largest score wins, the first in order on a tie (so a winner exists iff one pair is not
 *      singular); pairs after one that scores U are not tried (they cannot win).
 *   6. S = the winner's inliers; fewer than 2: no point.  X = step 3 over S.  Then at most `rounds` (0 .. 4) times: S' = the
 *      inliers of X; stop if S' == S; no point if |S'| < 2; S = S', X = step 3 over S.  The reported inliers are those of
 *      the final X; fewer than 2: no point.
 *   7. Parallax, two sweeps over the final inliers: a0 = the first inlier, a = the inlier with the smallest u_a0 . u_i (the
 *      lowest position on a tie), and the reported cosine = the smallest u_a . u_i.  Exact for two inliers, otherwise a
 *      lower bound of the largest pairwise angle in O(inliers).  (A dot product that is a NaN counts as 2.)
 * Outputs: d_points f32 [track_capacity][4] = X, Y, Z and the parallax cosine, {0, 0, 0, 2} for no point (the pose call's
 * "none" row); d_stats uint32 [track_capacity][4] = {U, inliers (0 for no point), reason, the winning pair as ci << 16 | cj
 * (candidate indices) or 0xFFFFFFFF when there is none}, reason 0: point, 1: U < 2, 2: every pair singular or a later solve
 * singular, 3: fewer than 2 inliers at some stage; optional d_err f32 [track_capacity][2] = the rms (the canonical sum of the
 * inliers' squared errors over their number, its root) and the largest inlier reprojection error in px, {0, 0} for no point;
 * optional d_obs_state uint32 [obs_capacity]: 0 not usable, 1 usable and no inlier, 2 inlier (a no-point track has 0 and 1
 * only).  Rows t >= T are untouched, and so are observation entries outside every track's range.  (Ranges that overlap, which
 * no track table has, leave d_obs_state's shared entries with either track's value.)
 * Every output bit depends on the track's own inputs alone: a track alone equals the track in any batch, a captured call
 * replays to the same bits, and tests/cpp/triangulate_twin.cpp (the same header under g++) gives them on the host.  Whatever
 * the arrays hold the call ends, and nothing at or beyond a capacity (+ 1 for the offsets), n_rows_total or n_images is
 * read or written.  track_capacity == 0 is LF_MKD_OK and writes nothing.
 * How (csrc/mkd_triangulate.hip): ONE launch sized from track_capacity (T is read on the device); a group of 4 lanes owns a
 * track, 16 tracks a wave; lane l is slot l, sums are combined by a ds_bpermute butterfly, counts by ballot and popcount; the
 * first 4 positions stay in registers, later ones are read again on every walk.  COST: a walk is ceil(L / 4) steps for a
 * track of L positions, and a track takes 1 + (pairs tried, at most 28) + (1 + rounds) + 3 walks.  ONE track of every row is
 * slow, as one edge of every link is in the pose call: its walks run on 4 lanes of one wave, and one track of 100 000
 * observations takes 220 ms, four times what numpy takes on the host (profiles/triangulate.md).  No
 * scratch, no LDS, no allocation, no atomic, nobody waits; asynchronous on `stream` (NULL: the handle's own), capturable.
 * LF_MKD_ERR_BAD_ARG, reported before any device is touched (the message starts with "triangulate_tracks_device: "): a null
 * handle; with track_capacity > 0 a null d_track_offsets, d_table_counts, d_points or d_stats, and with obs_capacity > 0 too a
 * null d_obs_row or d_obs_image, a null d_kps with n_rows_total > 0, a null d_intrinsics or d_poses with n_images > 0;
 * max_reproj_px not finite or <= 0; rounds > 4; flags other than 0 (none is defined); d_track_offsets not 8-byte or any other
 * array not 4-byte aligned; n_rows_total, track_capacity or obs_capacity above 2^31 - 1. */
int lf_mkd_triangulate_tracks_device(lf_mkd *h, const lf_mkd_keypoint *d_kps, uint64_t n_rows_total, const uint64_t *d_track_offsets,
                                     uint64_t track_capacity, const int32_t *d_obs_row, const uint32_t *d_obs_image,
                                     uint64_t obs_capacity, const uint32_t *d_table_counts, const float *d_intrinsics,
                                     const float *d_poses, uint32_t n_images, float max_reproj_px, uint32_t rounds, uint32_t flags,
                                     float *d_points, uint32_t *d_stats, float *d_err, uint32_t *d_obs_state, void *stream);
/* Host pointers, synchronous: the same arrays on the host, track_offsets [n_tracks + 1], obs_row and obs_image [n_obs] (the
 * counts are n_tracks and n_obs), points [n_tracks][4], stats [n_tracks][4], optional err [n_tracks][2] and obs_state [n_obs]
 * (in and out: entries outside every range come back as they were).  Everything goes through the device call.
 * LF_MKD_ERR_BAD_ARG ("triangulate_tracks: "): a null handle or required pointer, max_reproj_px not finite or <= 0, rounds > 4,
 * flags other than 0, a total above 2^31 - 1. */
int lf_mkd_triangulate_tracks(lf_mkd *h, const lf_mkd_keypoint *kps, uint64_t n_rows_total, const uint64_t *track_offsets,
                              uint64_t n_tracks, const int32_t *obs_row, const uint32_t *obs_image, uint64_t n_obs,
                              const float *intrinsics, const float *poses, uint32_t n_images, float max_reproj_px, uint32_t rounds,
                              uint32_t flags, float *points, uint32_t *stats, float *err, uint32_t *obs_state);

/* lf_mkd_resect_cameras_device gives images that are not registered yet their ABSOLUTE POSE [R | t] (resection, PnP) from the
 * 2-D keypoints they own in tracks that already have a 3-D point: the step that fills the all-zero rows of d_poses that
 * lf_mkd_triangulate_tracks_device skips, so incremental structure from motion runs triangulate, resect, triangulate, ..
 * on the device.  Three launches, nothing read back.
 * Reads: the pool keypoints (x and y alone) and d_image_offsets [n_images + 1] (image i's rows are [d_image_offsets[i],
 * d_image_offsets[i + 1]), both ends clamped to n_rows_total, an inverted range empty); d_row_track [n_rows_total] as
 * lf_mkd_track_table_device writes it (the table index of a row's track or -1); d_points [track_capacity][4] as the
 * triangulation call writes it; T = min(d_table_counts[0], track_capacity); d_intrinsics [n_images][4] and d_poses
 * [n_images][12] as there (R row-major, then t; world to camera).
 * Row r of image i is a CORRESPONDENCE iff 0 <= d_row_track[r] < T, that track's d_points row has finite X, Y, Z and a fourth
 * value w <= cmin (cmin = cos(min_parallax_deg), formed once on the host in double: 0 degrees admits every real point, the
 * "none" row {0, 0, 0, 2} and a NaN fail), and the keypoint's x and y are finite.  M = their number; their POSITION 0 .. M - 1
 * is their ascending row order.  Image i is a CANDIDATE iff its intrinsics are finite with fx, fy > 0, its 12 values of d_poses
 * are finite, and R there is all zero or LF_MKD_RESECT_ALL is set.  Every other image's pose is copied to d_poses_out
 * unchanged, with d_stats = {0, 0, 1, 0xFFFFFFFF} and d_err = {0, 0}.
 * d_poses_out MAY be d_poses (in place): the first launch writes each image's candidacy into scratch, and the last launch,
 * the only one that stores to d_poses_out, decides from that flag; each of its workgroups reads and writes its own image's row
 * alone.
 * The algorithm, exactly (f64, + - * / and sqrt alone, contraction off, the order csrc/mkd_resect_math.h fixes; thr2 =
 * max_reproj_px^2 formed once on the host in double; the world points are d_points' f32 widened):
 *   1. BEARING of a keypoint: xn = ((x - cx) / fx, (y - cy) / fy, 1), f = xn / sqrt(xn.xn).
 *   2. SAMPLE k (0 <= k < n_samples) of image i draws 3 distinct positions with the verifiers' splitmix64 counter sampler:
 *      key = (uint64(seed + i) << 32) ^ (k << 6), draw t = 0 .. 63 is r = splitmix64(key ^ t), pos = ((r >> 32) * M) >> 32,
 *      a position already drawn is passed over; no sample if M < 3 or 64 draws give fewer than 3.  It is keyed on the image
 *      id, so an image's result depends on neither its neighbours in the call nor on n_images.
 *   3. P3P by Grunert's quartic (Haralick et al., Int. J. Computer Vision 13(3), 1994): with X1, X2, X3 the sample's points in
 *      draw order, a = |X2 - X3|, b = |X1 - X3|, c = |X1 - X2|, ca = f2.f3, cb = f1.f3, cg = f1.f2, p = (a^2 - c^2) / b^2 and
 *      q = (a^2 + c^2) / b^2,
 *        A4 = (p - 1)^2 - 4 (c^2 / b^2) ca^2
 *        A3 = 4 [p (1 - p) cb - (1 - q) ca cg + 2 (c^2 / b^2) ca^2 cb]
 *        A2 = 2 [p^2 - 1 + 2 p^2 cb^2 + 2 ((b^2 - c^2) / b^2) ca^2 - 4 q ca cb cg + 2 ((b^2 - a^2) / b^2) cg^2]
 *        A1 = 4 [-p (1 + p) cb + 2 (a^2 / b^2) cg^2 cb - (1 - q) ca cg]
 *        A0 = (1 + p)^2 - 4 (a^2 / b^2) cg^2.
 *      The sample is INVALID iff not (|(X2 - X1) x (X3 - X1)|^2 > 1e-12 c^2 b^2) (kRsCollinear: a guard against exactly
 *      degenerate triangles -- it is sin^2 of the angle at X1, so it trips below about 1e-6 rad -- not a quality gate), or not
 *      (|A4| > 2^-20 max |A0 .. A3|) (kRsLeadRel, the F verifier's: a vanishing leading coefficient sends a root to infinity),
 *      or a coefficient is not finite.
 *      The real roots inside the Cauchy bound B = 1 + max |A0 .. A3| / |A4| come from one fixed-iteration finder: the
 *      breakpoints of a polynomial are -B, its derivative's real roots (recursively: the quadratic in closed form, q =
 *      -(b + sign(b) sqrt(disc)) / 2, roots q / a and c / q; then the cubic; then the quartic) and B; an interval whose ends
 *      differ in (value > 0) is halved kRsBisect = 64 times, then kRsNewton = 4 Newton steps from its middle, each taken iff
 *      it stays inside the interval.  Roots are taken in ascending order; root j (0 .. 3) of sample k is candidate c = 4 k + j.
 *      For a root v: u = ((p - 1) v^2 - 2 p cb v + 1 + p) / (2 (cg - v ca)); the candidate is skipped unless v > 0, that
 *      denominator is not 0, u > 0 and the pose below is finite.  s1 = sqrt(b^2 / (1 + v^2 - 2 v cb)), s2 = u s1, s3 = v s1,
 *      Yi = si fi.  The pose aligns the triangles' frames: e1 = (P2 - P1) / |.|, e3 = e1 x (P3 - P1) normalised, e2 = e3 x e1
 *      for P = X and P = Y; R = F_Y F_X^T (F's columns e1, e2, e3), t = Y1 - R X1.
 *   4. A correspondence is an INLIER of (R, t) by the triangulation call's rule: p = R X + t (each row summed left to right),
 *      p_z > 0 and ex^2 + ey^2 <= thr2, ex = fx (p_x / p_z) + cx - x, ey likewise.  A candidate's SCORE is its inliers among
 *      all M; the largest wins, the lowest c on a tie; without a candidate there is no pose.
 *   5. REFIT, at most `rounds` (0 .. 4) Gauss-Newton steps on the reprojection error: over the inliers S of the current pose
 *      the 21 + 6 sums of J^T J and J^T e for the step (w, dt) with R' = C(w) R, t' = t + dt and the rational Cayley map C(w) =
 *      ((1 - w.w) I + 2 w w^T + 2 [w]x) / (1 + w.w) (J from C(w) = I + 2 [w]x + ..); the 6 x 6 system by Cholesky, a pivot
 *      that is not positive ends the refit; the step is kept iff its MSAC cost -- the sum over all M of min(e^2, thr2), thr2
 *      for a point not in front -- is not above the current pose's, and the refit ends with the first step not kept.
 *   6. Every floating-point sum over correspondences is the CANONICAL SUM, the verifiers' block sum made part of the
 *      contract: 256 slots; slot s adds, from +0.0 and in ascending position, the positions with position mod 256 == s (a
 *      skipped position adds nothing); the 64 slots of a wave combine by the butterfly over slot xor 32, 16, .. 1; the four
 *      wave sums add as ((w0 + w1) + w2) + w3.
 *   7. The pose is rounded to f32; inliers, errors and states are those of the ROUNDED pose under step 4's test as the
 *      triangulation call evaluates it, so a following lf_mkd_triangulate_tracks_device sees exactly the inliers this call
 *      reports.  The pose is written iff their number is at least max(min_inliers, 3); otherwise the image's row of
 *      d_poses_out is all zero.
 * Outputs: d_poses_out f32 [n_images][12]; d_stats uint32 [n_images][4] = {M, inliers (0: no pose), reason, the winning c or
 * 0xFFFFFFFF when there is none}, reason 0: pose, 1: not a candidate (copied through, M reported as 0), 2: M < 3 or no
 * candidate from any sample, 3: fewer than the minimum inliers; optional d_err f32 [n_images][2] = the rms (the canonical sum
 * of the inliers' squared errors over their number, its root) and the largest inlier error in px, {0, 0} without a pose;
 * optional d_row_state uint32 [n_rows_total], written only in the ranges of the CANDIDATE images: 0 no correspondence, 1
 * correspondence, 2 inlier (a no-pose image has 0 and 1 only); every other entry is untouched.  (Ranges that overlap, which no
 * pool has, leave shared entries with either image's value.)
 * Every output bit depends on the image's own inputs, its id and the seed alone: an image alone equals the image in any batch
 * at the same id, a captured call replays to the same bits, and tests/cpp/resect_twin.cpp (the same header under g++) gives
 * them on the host.  Whatever the arrays hold the call ends, and nothing at or beyond n_rows_total, track_capacity or n_images
 * (+ 1 for the offsets) is read or written.  n_images == 0 is LF_MKD_OK and writes nothing.
 * How (csrc/mkd_resect.hip): rs_gather, a workgroup per image, compacts the correspondences' rows in order into scratch;
 * rs_score, image x 256 candidates x slice of positions, one candidate per lane, the correspondences staged in LDS, integer
 * atomic adds of the counts; rs_select, a workgroup per image, the argmax, the refit as block passes, the outputs.  Scratch
 * (4 bytes a row, 8 an image, 16 per image and sample) belongs to the handle and grows only when a call asks for more: a
 * warmed-up call allocates nothing and is capturable (a later call that asks for MORE replaces the scratch, and a graph captured
 * before it names the old one: capture after the largest call); asynchronous on `stream` (NULL: the handle's own).  COST: one image
 * owning every row is walked by ONE workgroup in rs_gather and rs_select (profiles/resect.md).
 * LF_MKD_ERR_BAD_ARG, reported before any device is touched (the message starts with "resect_cameras_device: "): a null
 * handle; with n_images > 0 a null d_image_offsets, d_table_counts, d_intrinsics, d_poses, d_poses_out or d_stats, with
 * n_rows_total > 0 too a null d_kps or d_row_track, and with track_capacity > 0 too a null d_points; flags other than
 * LF_MKD_RESECT_ALL; max_reproj_px not finite or <= 0; min_parallax_deg outside [0, 180] or a NaN; n_samples 0 or above 4096;
 * rounds > 4; d_image_offsets not 8-byte or any other array not 4-byte aligned; n_images, n_rows_total or track_capacity above
 * 2^31 - 1. */
#define LF_MKD_RESECT_ALL (1u)   /* resect registered images too (re-estimate them from the points) */
int lf_mkd_resect_cameras_device(lf_mkd *h, const lf_mkd_keypoint *d_kps, const uint64_t *d_image_offsets, uint32_t n_images,
                                 uint64_t n_rows_total, const int32_t *d_row_track, const float *d_points, uint64_t track_capacity,
                                 const uint32_t *d_table_counts, const float *d_intrinsics, const float *d_poses,
                                 float max_reproj_px, float min_parallax_deg, uint32_t n_samples, uint32_t min_inliers,
                                 uint32_t rounds, uint32_t seed, uint32_t flags, float *d_poses_out, uint32_t *d_stats, float *d_err,
                                 uint32_t *d_row_state, void *stream);
/* Host pointers, synchronous, ONE image: kps [n_rows] are its rows, row_track [n_rows], points [n_tracks][4] (every row of
 * it is read: T = n_tracks), intrinsics [4]; pose [12], stats [4], optional err [2] and row_state [n_rows].  The image is
 * image 0 of a device call with an all-zero pose, so it is always a candidate; pass seed + i to get image i of a batch.
 * Everything goes through the device call.  LF_MKD_ERR_BAD_ARG ("resect_camera: "): a null handle or required pointer, the
 * scalars as above, a total above 2^31 - 1. */
int lf_mkd_resect_camera(lf_mkd *h, const lf_mkd_keypoint *kps, uint64_t n_rows, const int32_t *row_track, const float *points,
                         uint64_t n_tracks, const float *intrinsics, float max_reproj_px, float min_parallax_deg,
                         uint32_t n_samples, uint32_t min_inliers, uint32_t rounds, uint32_t seed, uint32_t flags, float *pose,
                         uint32_t *stats, float *err, uint32_t *row_state);

/* lf_mkd_track_descriptors_device gives a reconstruction DESCRIPTORS OF ITS OWN: per track of a track table one 8-bit row, the
 * sum of its observations' rows normalised and quantised again.  With them a photograph that was not part of the collection is
 * localised by two calls that exist: lf_mkd_match_q8_device of its rows (a) against the track rows (b, nb = track_capacity)
 * returns per row a table index or -1, which is the d_row_track that lf_mkd_resect_cameras_device reads.  The model is
 * track_capacity x 128 bytes and the points; the pool's rows need not stay resident.  One launch, nothing read back.
 * Reads: d_q uint8 [n_rows_total][128], the pool's rows as lf_mkd_quantize_descriptors_device writes them (byte = q + 128);
 * the track table d_track_offsets [track_capacity + 1], d_obs_row [obs_capacity] and d_table_counts exactly as
 * lf_mkd_triangulate_tracks_device reads them (T = min(d_table_counts[0], track_capacity) and O = min(d_table_counts[1],
 * obs_capacity) are formed on the device; track t's positions are [d_track_offsets[t], d_track_offsets[t + 1]), both ends
 * clamped to O, an inverted range empty); optional d_obs_state uint32 [obs_capacity], the states triangulation and bundle
 * adjustment write, with min_state 0 .. 2 (NULL: min_state is not looked at); optional d_points f32 [track_capacity][4] as the
 * triangulation call writes it, with min_parallax_deg (NULL: it is not looked at); scale, the quantiser's (0: 256).
 * The contract, exactly:
 *   1. Of a track only its first 65 536 positions are read.  Such a position k CONTRIBUTES iff d_obs_state is NULL or
 *      d_obs_state[k] >= min_state, and 0 <= d_obs_row[k] < n_rows_total.  C = the contributors' number.
 *   2. S_k = the sum over the contributors of (byte_k - 128), k = 0 .. 127, and n2 = sum_k S_k^2: integers, whatever bytes the
 *      rows hold (a byte 0 counts as -128).  With at most 65 536 contributors |S_k| < 2^23 and n2 < 2^53: int64 and f64 hold
 *      every one of them exactly, and no order of summation changes them.
 *   3. Track t < T is DESCRIBED iff d_points is NULL or its row there passes resection's rule: finite X, Y, Z and a fourth
 *      value w <= cmin, cmin = cos(min_parallax_deg) formed once on the host in double (the "none" row {0, 0, 0, 2} and a NaN
 *      fail).
 *   4. If the track is described, C > 0 and n2 > 0: v_k = ((double)S_k * (double)scale) / sqrt((double)n2) -- the product is
 *      exact, sqrt and / are one correctly rounded f64 operation each, contraction off -- q_k = clamp(rint(v_k), -127, 127),
 *      ties to even, and the row's byte k = q_k + 128.  (|v| = scale: it is the quantiser's row of S / |S|.)
 *   5. In every other case -- not described, no contributor, sums that cancel -- and for the rows T .. track_capacity - 1 the
 *      row is the ZERO ROW, all bytes 128: its similarity with every row is 0, so the ratio test passes it only where every
 *      other similarity is negative, and resection refuses a track without a point anyway.  Exactly track_capacity rows are
 *      written: the matcher takes nb = track_capacity, and no count is read back.
 * Outputs: d_desc uint8 [track_capacity][128]; optional d_desc_stats int32 [track_capacity][2] = {C, spread}: C as in 1 (for
 * a track that is not described too; 0 for the rows from T on), spread = the smallest over the contributors of sum_k (byte_k -
 * 128) q_k, their similarity with the row as the matcher would score it -- small where a track fuses two things --, and
 * INT32_MIN for a zero row.
 * Every output bit depends on the track's own inputs alone: not on the run, the CU count, the grid or the track's place in
 * the table; a captured call replays to the same bytes, and tests/cpp/track_desc_twin.cpp (csrc/mkd_track_desc_math.h under
 * g++) gives them on the host.  Whatever the arrays hold the call ends, and nothing at or beyond n_rows_total,
 * track_capacity (+ 1 for the offsets) or obs_capacity is read or written.  track_capacity == 0 is LF_MKD_OK and writes nothing.
 * How (csrc/mkd_track_desc.hip): ONE launch sized from track_capacity; a group of 8 lanes owns a track and a lane 16 bytes of
 * the row, so a contributor's row is one 128-byte request; the walk issues the loads of 4 positions before it adds the
 * first; 16 integer accumulators a lane, n2 by a butterfly within the group; with d_desc_stats a second walk over the same
 * rows.  A track of more than 256 positions is taken by its whole wave, group g walking every eighth position.  COST: ONE
 * track with every row is walked by one wave, 65 536 positions at the most: 1.96 ms, where the torch route takes 1.33 ms
 * (profiles/track_descriptors.md).  No scratch, no
 * LDS, no allocation, no atomic, nobody waits; asynchronous on `stream` (NULL: the handle's own), capturable.
 * LF_MKD_ERR_BAD_ARG, reported before any device is touched (the message starts with "track_descriptors_device: "): a null
 * handle; with track_capacity > 0 a null d_track_offsets, d_table_counts or d_desc, with obs_capacity > 0 too a null
 * d_obs_row, and with n_rows_total > 0 too a null d_q; min_state > 2; min_parallax_deg outside [0, 180] or a NaN; scale
 * negative, not finite or subnormal; d_q or d_desc not 16-byte, d_track_offsets not 8-byte or any other array not 4-byte
 * aligned; n_rows_total, track_capacity or obs_capacity above 2^31 - 1. */
int lf_mkd_track_descriptors_device(lf_mkd *h, const uint8_t *d_q, uint64_t n_rows_total, const uint64_t *d_track_offsets,
                                    uint64_t track_capacity, const int32_t *d_obs_row, uint64_t obs_capacity,
                                    const uint32_t *d_table_counts, const uint32_t *d_obs_state, uint32_t min_state,
                                    const float *d_points, float min_parallax_deg, float scale, uint8_t *d_desc,
                                    int32_t *d_desc_stats, void *stream);
/* Host pointers, synchronous: the same arrays on the host, track_offsets [n_tracks + 1] and obs_row [n_obs] (the counts are
 * n_tracks and n_obs), optional obs_state [n_obs] and points [n_tracks][4]; desc [n_tracks][128], optional desc_stats
 * [n_tracks][2].  Everything goes through the device call.  LF_MKD_ERR_BAD_ARG ("track_descriptors: "): a null handle or
 * required pointer, the scalars as above, a total above 2^31 - 1. */
int lf_mkd_track_descriptors(lf_mkd *h, const uint8_t *q, uint64_t n_rows_total, const uint64_t *track_offsets, uint64_t n_tracks,
                             const int32_t *obs_row, uint64_t n_obs, const uint32_t *obs_state, uint32_t min_state,
                             const float *points, float min_parallax_deg, float scale, uint8_t *desc, int32_t *desc_stats);

/* lf_mkd_bundle_adjust_device refines the registered cameras and the tracks' points JOINTLY (bundle adjustment): Levenberg-
 * Marquardt on the reprojection error over all free cameras (6 parameters each, intrinsics fixed) and all free points, the
 * reduced camera system solved matrix-free by preconditioned conjugate gradients.  It is what closes the triangulate / resect
 * loop, whose every step is conditioned on the one before it.  Nothing is read back.
 * Inputs are what the three calls above take and leave: d_kps, n_rows_total and d_image_offsets [n_images + 1] (the pooled
 * rows), the track table (d_track_offsets, track_capacity, d_obs_row, d_obs_image, obs_capacity, d_table_counts = {T, O},
 * both clamped to the capacities), d_points [track_capacity][4] (X, Y, Z and the cosine the triangulation call writes),
 * d_intrinsics [n_images][4], d_poses [n_images][12]; optional d_obs_state [obs_capacity] (the triangulation call's) and
 * d_camera_fixed uint32 [n_images] (non-zero: the pose is held; hold two cameras, or one and a distance, to fix the gauge).
 * Outputs: d_poses_out [n_images][12] (may be d_poses), d_points_out [track_capacity][4] (may be d_points), optional
 * d_obs_state_out [obs_capacity] (may be d_obs_state), d_trace f64 [iterations][8], d_counts uint32 [4].
 * The algorithm, exactly (f64, + - * / and sqrt alone, contraction off, the order csrc/mkd_bundle_math.h fixes; thr2 =
 * max_reproj_px^2 and tol2 = cg_tol^2 formed in double from the f32 arguments):
 *   1. Position p of track j < T is ACTIVE, for the whole call, iff it is usable by the triangulation call's rule (row and
 *      image in range, a usable camera, a finite keypoint), its row lies inside its image's range of d_image_offsets (clamped
 *      to n_rows_total as resection clamps it), the track's INPUT row of d_points has finite X, Y, Z and a fourth value <= 1,
 *      and d_obs_state is null or d_obs_state[p] == 2.  The first launches build, in the handle's scratch, the inverse map
 *      row -> (position, track) and each image's ascending list of active rows.  A row named by two tracks takes either;
 *      track ranges or image ranges that overlap (no table has them) leave the result unspecified, within every bound.
 *   2. A camera is FREE iff it is registered (usable by the triangulation call's rule) and d_camera_fixed is null or zero
 *      there; a point is FREE iff its track has an active position.  Everything else is constant.  The state is f64, widened
 *      from the f32 inputs; lambda = lambda0.
 *   3. Per iteration k: an active observation is an INLIER iff p_z > 0 and e^2 <= thr2 at the state; outliers add nothing to
 *      the normal equations.  Its camera rows Jx, Jy are resection's (step 5 there); its point rows are (a, 0, gx) R and
 *      (0, b, gy) R.  Per point V (6 distinct entries) and g_p (3) are summed in the triangulation call's 4-slot order over
 *      the track's positions (slot = (p - lo) mod 4, ascending, then (s0 + s2) + (s1 + s3)); per camera U (21) and g_c (6)
 *      in resection's 256-slot order over the image's list.  cost_k = the MSAC terms (min(e^2, thr2); thr2 when not in
 *      front) of all active observations, per track in the 4-slot order, then over the track index in the 256-slot order.
 *   4. lambda max(d, 1e-6) is added to every diagonal entry d of U and V.  A free camera whose damped U* fails the Cholesky
 *      pivot test is HELD for this iteration; so is a free point with fewer than 2 inliers or whose V* is singular by the
 *      triangulation call's determinant rule.  Held items take a zero step, and the coupling W = J_c^T J_p of an observation
 *      enters only if it is an inlier whose camera and point are both free and not held.
 *   5. (U* - W V*^-1 W^T) x = g_c - W V*^-1 g_p by PCG from x = 0, preconditioned by U*^-1 (Cholesky).  The operator is two
 *      passes: per track y_j = V*^-1 (the 4-slot sum of W^T p), per image U* p - (the 256-slot sum of W y).  A global dot
 *      product is the 256-slot sum over the image id of the per-image 6-term dots (left to right).  A step: alpha = r.z /
 *      p.Ap, x += alpha p, r -= alpha Ap, z = U*^-1 r, beta = r.z' / r.z, p = z + beta p.  CG stops for good, later steps
 *      being no-ops, at the first step where not (p.Ap > 0) (before x moves) or, after x moved, not (r.z' > 0) or r.z' <=
 *      tol2 r.z0.  The trace counts the steps that moved x.
 *   6. dp_j = V*^-1 (g_p - sum W^T x); the candidate is resection's Cayley update by x per camera and X - dp per point.
 *      cost' = step 3's cost at the candidate.  ACCEPT iff cost' <= cost_k (a NaN fails): the state becomes the candidate and
 *      lambda = max(lambda / 4, 2^-40); else the state stays and lambda = min(8 lambda, 2^40).  Always `iterations` of them.
 *   7. Free cameras are rounded to f32 into d_poses_out, every other image's 12 words are copied; free points are rounded
 *      into d_points_out [.][0 .. 2], the fourth word and every other row below T are copied, rows >= T are untouched.
 *      d_obs_state_out (positions inside a track's range): 0 inactive, 1 active, 2 inlier of the ROUNDED state under the
 *      triangulation call's test.  d_trace [k] = {cost_k, cost', the lambda used, accepted, CG steps, inliers, held cameras,
 *      held points}; d_counts = {free cameras, free points, active observations, accepted steps}.
 * A call with nothing free, or with T == 0, copies its inputs through bit for bit.  n_images == 0 is LF_MKD_OK and writes
 * nothing.  Whatever the arrays hold the call ends, and nothing at or beyond a capacity is read or written.
 * tests/cpp/bundle_twin.cpp (the same header under g++) gives every output word on the host.
 * How (csrc/mkd_bundle.hip): 5 + iterations x (6 + 5 cg_iterations) launches fixed by the scalars alone, a linear sequence
 * (capturable once warmed up; capture after the largest call, as for resection).  4 lanes own a track, a workgroup owns an
 * image, ONE workgroup does each global sum and the CG scalars; no floating-point atomic, nobody waits for another workgroup.
 * W is formed again at every use, not stored (measured faster: profiles/bundle.md).  Scratch (4 bytes a position of
 * obs_capacity, 156 a track, 664 an image, 12 a row) belongs to the handle and grows only when a call asks for more.  COST: one image owning every row is walked by ONE workgroup in
 * both per-image kernels, M / 256 rounds each (profiles/bundle.md).  Asynchronous on `stream` (NULL: the handle's own).
 * LF_MKD_ERR_BAD_ARG, reported before any device is touched (the message starts with "bundle_adjust_device: "): a null
 * handle; with n_images > 0 a null d_image_offsets, d_table_counts, d_intrinsics, d_poses, d_poses_out, d_trace or d_counts,
 * with track_capacity > 0 too a null d_track_offsets, d_points or d_points_out, with obs_capacity > 0 too a null d_obs_row or
 * d_obs_image, and with n_rows_total > 0 too a null d_kps; non-zero flags; max_reproj_px or lambda0 not finite or <= 0;
 * iterations 0 or above 64; cg_iterations 0 or above 256; cg_tol outside [0, 1) or a NaN; d_image_offsets, d_track_offsets
 * or d_trace not 8-byte or any other array not 4-byte aligned; a total or a capacity above 2^31 - 1. */
int lf_mkd_bundle_adjust_device(lf_mkd *h, const lf_mkd_keypoint *d_kps, const uint64_t *d_image_offsets, uint32_t n_images,
                                uint64_t n_rows_total, const uint64_t *d_track_offsets, uint64_t track_capacity,
                                const int32_t *d_obs_row, const uint32_t *d_obs_image, uint64_t obs_capacity,
                                const uint32_t *d_table_counts, const float *d_points, const float *d_intrinsics,
                                const float *d_poses, const uint32_t *d_obs_state, const uint32_t *d_camera_fixed,
                                float max_reproj_px, float lambda0, uint32_t iterations, uint32_t cg_iterations, float cg_tol,
                                uint32_t flags, float *d_poses_out, float *d_points_out, uint32_t *d_obs_state_out,
                                double *d_trace, uint32_t *d_counts, void *stream);
/* Host pointers, synchronous: the same arrays with T = n_tracks and O = n_obs; poses_out [n_images][12], points_out
 * [n_tracks][4], optional obs_state_out [n_obs] (entries outside every track's range come back 0), trace [iterations][8],
 * counts [4].  Everything goes through the device call.  LF_MKD_ERR_BAD_ARG ("bundle_adjust: "): a null handle or required
 * pointer, the scalars as above, a total above 2^31 - 1. */
int lf_mkd_bundle_adjust(lf_mkd *h, const lf_mkd_keypoint *kps, const uint64_t *image_offsets, uint32_t n_images,
                         uint64_t n_rows_total, const uint64_t *track_offsets, uint64_t n_tracks, const int32_t *obs_row,
                         const uint32_t *obs_image, uint64_t n_obs, const float *points, const float *intrinsics,
                         const float *poses, const uint32_t *obs_state, const uint32_t *camera_fixed, float max_reproj_px,
                         float lambda0, uint32_t iterations, uint32_t cg_iterations, float cg_tol, uint32_t flags,
                         float *poses_out, float *points_out, uint32_t *obs_state_out, double *trace, uint32_t *counts);

/* lf_mkd_bundle_adjust_intrinsics_device is lf_mkd_bundle_adjust_device with the intrinsics of the images that share a lens
 * REFINED beside the poses and the points (self-calibration).  Every input of that call in its order up to d_camera_fixed,
 * then d_camera_group uint32 [n_images] (the lens an image was taken with; null: every image is in group 0 and n_groups must
 * be 1; an id >= n_groups: the image's intrinsics are constant), n_groups, and refine = LF_MKD_BA_REFINE_FOCAL |
 * LF_MKD_BA_REFINE_PRINCIPAL.  Group g has three parameters (s, dx, dy), (1, 0, 0) at the start; image i of the group has
 * fx = s fx0_i, fy = s fy0_i, cx = cx0_i + dx, cy = cy0_i + dy (fx0 .. the f32 input widened), so the aspect ratio and the
 * images' differences are kept.  A parameter refine does not name stays at its start.
 * Outputs: the sibling's, with d_trace f64 [iterations][9] and d_counts uint32 [5], and d_intrinsics_out [n_images][4] (may be
 * d_intrinsics), optional d_group_out [n_groups][3].
 * The algorithm is the sibling's seven steps with these additions, exactly (csrc/mkd_bundle_math.h):
 *   2. A group is FREE iff refine != 0 and one of its images is usable and has an active row (a camera held by d_camera_fixed
 *      informs its group all the same: every camera fixed is calibration under known poses).  The intrinsics an observation
 *      is read under are f64: for an image of a free group the products above of the group's state, else the input widened.
 *   3. An inlier's group rows are J_k = d e / d (s, dx, dy) = ((fx0 u, 1, 0), (fy0 v, 0, 1)), (u, v) = (p_x / p_z, p_y / p_z),
 *      a column refine does not name being zero.  Per usable image of a free group, in the 256-slot order over the image's
 *      list: U_kk = J_k^T J_k (6 distinct) and g_k = J_k^T e (3), the inlier count, and (free cameras) U_ck = J_c^T J_k
 *      (18); per group those nine and the count are then summed over the group's usable images in the 256-slot order over
 *      the image id (slot = id mod 256).
 *   4. U_kk gets lambda max(d, 1e-6) on its diagonal, then the rows and columns of the parameters not refined are replaced by
 *      the identity's, scaled by a refined parameter's damped entry (s's for dx and dy, dx's for s: the determinant test
 *      compares magnitudes), with a zero right-hand side; a free group with no inlier or whose block is singular by the triangulation call's determinant rule is
 *      HELD for the iteration.  The block U_ck enters iff camera and group both move (free, not held); the coupling W_k =
 *      J_k^T J_p of an inlier enters iff its group and its point both move, whatever its camera.
 *   5. The unknowns are the free cameras' 6 and the free groups' 3; the right-hand side of a group is g_k - (the sum of
 *      W_k y, y = V*^-1 g_p, per image then per group in the two orders above); the preconditioner is block-Jacobi, U*^-1
 *      per camera and U_kk*^-1 per group (the cofactor solve).  The operator: per track y_j = V*^-1 (the 4-slot sum of, per
 *      position, W^T p_c + W_k^T p_k, or the one of them that enters); per image Ap_c = (U* p_c + U_ck p_k) - (the sum of W y) and
 *      the image's share (U_ck^T p_c, or 0 for a camera that does not move) - (the sum of W_k y); per group Ap_k = U_kk* p_k +
 *      (the sum of its images' shares over the image id).  A global dot product is the 256-slot sum over the image id of
 *      the cameras' dots plus the 256-slot sum over the group id of the groups' 3-term dots, in that order.
 *   6. dp_j = V*^-1 (g_p - the same sum with x); a moving group's candidate is (s, dx, dy) - x_k in the parameters refined.  A
 *      candidate in which a moving group's s is not finite or not > 0 is REJECTED whatever its cost (the trace still shows
 *      the cost computed).
 *   7. d_intrinsics_out: for an image of a free group the f64 products rounded to f32, else the input's four words;
 *      d_group_out [g] = the state rounded, (1, 0, 0) for a group that is not free.  d_obs_state_out is judged under the
 *      rounded poses, points AND d_intrinsics_out, so lf_mkd_triangulate_tracks_device's test with them agrees.  d_trace [k]
 *      [8] = held groups; d_counts [4] = free groups.
 * With refine == 0 no group is free and every word this call shares with lf_mkd_bundle_adjust_device is that call's, bit for
 * bit (the widened intrinsics give the same bits); d_intrinsics_out is then a copy.  tests/cpp/bundle_intr_twin.cpp gives
 * every output word on the host.
 * How (csrc/mkd_bundle.hip): the sibling's kernels in their double-intrinsics form plus three with a workgroup per group:
 * 6 + iterations x (7 + 6 cg_iterations) launches fixed by the scalars alone, capturable once warmed up; no floating-point
 * atomic, nobody waits for another workgroup, no kernel spills.  Scratch is the sibling's plus 244 bytes an image and 252 a
 * group, the handle's.  COST: each per-group workgroup walks ALL image ids, so a group sum costs n_groups x n_images reads a
 * CG step: fine for the few lenses of a collection, quadratic with a group per image (profiles/bundle_intrinsics.md); the
 * per-image kernels now also walk every usable fixed image of a free group.
 * LF_MKD_ERR_BAD_ARG, before any device is touched ("bundle_adjust_intrinsics_device: "): the sibling's list in its order
 * with a null d_intrinsics_out among the required pointers; then refine above 3; n_groups == 0 with n_images > 0, or a null
 * d_camera_group with n_groups != 1; then the scalars, the alignment (d_camera_group, d_intrinsics_out and d_group_out 4-byte)
 * and the totals (n_groups too) as there. */
#define LF_MKD_BA_REFINE_FOCAL (1u)       /* refine every free group's focal scale s */
#define LF_MKD_BA_REFINE_PRINCIPAL (2u)   /* refine every free group's principal-point shift (dx, dy) */
int lf_mkd_bundle_adjust_intrinsics_device(lf_mkd *h, const lf_mkd_keypoint *d_kps, const uint64_t *d_image_offsets, uint32_t n_images,
                                           uint64_t n_rows_total, const uint64_t *d_track_offsets, uint64_t track_capacity,
                                           const int32_t *d_obs_row, const uint32_t *d_obs_image, uint64_t obs_capacity,
                                           const uint32_t *d_table_counts, const float *d_points, const float *d_intrinsics,
                                           const float *d_poses, const uint32_t *d_obs_state, const uint32_t *d_camera_fixed,
                                           const uint32_t *d_camera_group, uint32_t n_groups, uint32_t refine, float max_reproj_px,
                                           float lambda0, uint32_t iterations, uint32_t cg_iterations, float cg_tol, uint32_t flags,
                                           float *d_poses_out, float *d_points_out, float *d_intrinsics_out, float *d_group_out,
                                           uint32_t *d_obs_state_out, double *d_trace, uint32_t *d_counts, void *stream);
/* Host pointers, synchronous, through the device call: the sibling's arrays, camera_group [n_images] or null,
 * intrinsics_out [n_images][4], optional group_out [n_groups][3], trace [iterations][9], counts [5].
 * LF_MKD_ERR_BAD_ARG ("bundle_adjust_intrinsics: "): as the device form, without the alignment. */
int lf_mkd_bundle_adjust_intrinsics(lf_mkd *h, const lf_mkd_keypoint *kps, const uint64_t *image_offsets, uint32_t n_images,
                                    uint64_t n_rows_total, const uint64_t *track_offsets, uint64_t n_tracks, const int32_t *obs_row,
                                    const uint32_t *obs_image, uint64_t n_obs, const float *points, const float *intrinsics,
                                    const float *poses, const uint32_t *obs_state, const uint32_t *camera_fixed,
                                    const uint32_t *camera_group, uint32_t n_groups, uint32_t refine, float max_reproj_px,
                                    float lambda0, uint32_t iterations, uint32_t cg_iterations, float cg_tol, uint32_t flags,
                                    float *poses_out, float *points_out, float *intrinsics_out, float *group_out,
                                    uint32_t *obs_state_out, double *trace, uint32_t *counts);

/* ---- geometric verification: RANSAC homography of matched keypoints ---------------------------------------------
 * For one pair of images, or for n_pairs independent pairs in one call: a homography H with b ~ H a fitted robustly to the
 * matches, and the matches that agree with it.  Inputs are what the entry points above produce: lf_mkd_keypoint rows and the
 * matcher's int32 match array (index into b, or -1).
 *   Pair p uses a rows [offsets_a[p], offsets_a[p+1]) and b rows [offsets_b[p], offsets_b[p+1]); match is indexed like a and
 *   its values are local to the pair's b rows (as lf_mkd_match_device writes them for that pair).  At most 2^31 - 1 rows per
 *   side of a pair.
 * Outputs: H [n_pairs][9] row-major, pixel coordinates, scaled so that H[8] = 1; verified (indexed like a) = match with every
 * non-inlier set to -1; stats [n_pairs][4] = {final inlier count, best hypothesis' inlier count, best hypothesis' index k
 * (0xFFFFFFFF: no valid hypothesis), M = matches considered}.
 * The algorithm, exactly (a CPU restatement reproduces every hypothesis: tests/homography_ref.py; an f32 twin of the kernel
 * reproduces every output bit: tests/homography_f32.py):
 *   1. Considered matches: i with 0 <= match[i] < nb_pair (anything else counts as -1); positions 0 .. M-1 list them by
 *      ascending i.  Both point sets are normalised over the considered matches: centroid at the origin, scale s such that
 *      the RMS distance from it is sqrt(2) (s = sqrt(2 M / sum of squared distances), 1 if that sum is 0).  Rows that are
 *      not considered are never read; a NaN or infinite coordinate in a considered row leaves the pair without a valid
 *      hypothesis (its normalised coordinates on that axis are all non-finite), so its outputs are those of step 6.
 *   2. Sampler: hypothesis k takes draws t = 0..31, r = splitmix64(((uint64)(seed + p) << 32) ^ ((uint64)k << 5) ^ t),
 *      pos = ((r >> 32) * M) >> 32, and keeps the first 4 distinct positions (fewer: the hypothesis is invalid).  splitmix64
 *      is the standard finaliser with the 0x9E3779B97F4A7C15 pre-increment.  A single-pair call with seed s + p therefore
 *      equals pair p of a batched call with seed s.
 *   3. Minimal solver, f32 on the normalised coordinates: invalid if either 4-point set has three points with
 *      |(p1 - p0) x (p2 - p0)| < 1e-4 (twice a triangle's area, for the four triples).  Else Heckbert's square -> quad maps A
 *      (samples in a) and B (samples in b), multiplied through by their denominators, and H = B adj(A), divided by its
 *      largest |entry|; invalid if that is not finite and positive, or if the samples' w = h3 . [x y 1] differ in sign.
 *      H is negated if they are negative (so that w > 0 for the samples), then taken to pixel coordinates (invalid if a
 *      value is not finite).
 *   4. Score: point i is an inlier of H if w > 0 and (bx - u/w)^2 + (by - v/w)^2 < threshold^2 (the forward transfer error;
 *      evaluated as (bx w - u)^2 + (by w - v)^2 < threshold^2 w^2).  The best hypothesis has the largest count; ties go to
 *      the smallest k.
 *   5. Refit (unless LF_MKD_VERIFY_NO_REFINE): least squares with h8 = 1 over the current H's inliers in the normalised
 *      coordinates of step 1 (the normal equations accumulated in f64 in a fixed order, solved by an 8x8 Cholesky
 *      factorisation; a pivot at or below 1e-12 of the largest diagonal element fails the refit), rescored as in step 4 (w > 0).
 *      A refit is judged by its truncated quadratic cost over the considered matches (MSAC: an inlier adds its squared
 *      transfer error, any other match threshold^2; summed in f64 in a fixed order) and kept if that cost is not above the
 *      current H's -- so a refit that fits the inliers better may give up a few matches that only the 4-point hypothesis
 *      admitted.  At most 3 rounds, stopping when the inlier set stops changing; a failed or rejected refit keeps the current H.
 *   6. M < 4, or no valid hypothesis: H all zero, verified all -1, final count 0; the status is LF_MKD_OK.
 * The bits of every output depend on the pair's inputs, seed + p, n_hypotheses, threshold and flags alone (not on n_pairs or
 * on the run).  Null pointers, n_hypotheses of 0 or above 65536 and a threshold that is not positive or whose f32 square
 * threshold * threshold is not a finite normal number (so 1.0842022e-19 <= threshold <= 1.8446743e19 as f32 values) are
 * LF_MKD_ERR_BAD_ARG; n_pairs == 0 is LF_MKD_OK and writes nothing.  flags: LF_MKD_VERIFY_NO_REFINE (below). */

/* Host pointers, one pair, synchronous. */
int lf_mkd_verify_homography(lf_mkd *h, const lf_mkd_keypoint *kps_a, uint64_t na,
                             const lf_mkd_keypoint *kps_b, uint64_t nb, const int32_t *match,
                             uint32_t n_hypotheses, float threshold_px, uint32_t seed, uint32_t flags,
                             float *H, int32_t *verified, uint32_t *stats);

/* Device pointers, n_pairs independent problems in one call, asynchronous on `stream` (NULL: the handle's own).  Both offset
 * arrays have n_pairs + 1 entries and live on the device.  Three launches, no host synchronisation, and no allocation once the
 * handle's scratch has grown to the largest n_pairs x n_hypotheses seen: a warmed-up call can be captured in a hipGraph.
 * The scratch belongs to the handle, so calls of one handle must be stream-ordered (one stream, or the caller orders them).
 * d_verified also holds each pair's list of considered rows between the call's launches: it must not overlap d_match or
 * either keypoint array (an in-place call with d_verified == d_match would overwrite its own input; the identical pointers
 * are refused with LF_MKD_ERR_BAD_ARG).  A call needs n_pairs x ceil(n_hypotheses / 256) x (its row slices, at most 16)
 * < 2^24 scoring workgroups; a larger one is LF_MKD_ERR_BAD_ARG. */
int lf_mkd_verify_homography_device(lf_mkd *h, const lf_mkd_keypoint *d_kps_a, const uint64_t *d_offsets_a,
                                    const lf_mkd_keypoint *d_kps_b, const uint64_t *d_offsets_b,
                                    const int32_t *d_match, uint32_t n_pairs, uint32_t n_hypotheses,
                                    float threshold_px, uint32_t seed, uint32_t flags,
                                    float *d_H, int32_t *d_verified, uint32_t *d_stats, void *stream);
/* ---- geometric verification: RANSAC fundamental matrix of matched keypoints --------------------------------------
 * The general two-view constraint b^T F a = 0 (a = (x, y, 1) in image a, b = (u, v, 1) in image b, pixels), fitted robustly
 * by 7-point RANSAC: for pairs with parallax (a 3-D scene seen from two places), where a homography keeps only the dominant
 * plane.  A scene that is (nearly) one plane leaves F underdetermined -- any F = [e]x H fits it -- so use the homography
 * for such pairs.  Inputs, pair layout, argument checks, n_pairs == 0, the 2^24-workgroup limit and the stream rules are
 * those of lf_mkd_verify_homography*; F and H verification share the handle's scratch, so calls of one handle (of either
 * kind) must be stream-ordered.  d_verified must not overlap d_match or the keypoints (d_verified == d_match is refused).
 * Outputs: F [n_pairs][9] row-major, pixel coordinates, divided by its entry of largest magnitude (the first in row-major
 * order on a tie), which is therefore exactly +1; verified = match with every non-inlier set to -1; stats [n_pairs][4] =
 * {final inlier count, best candidate's inlier count, best candidate's index c = 3 k + j (k the sample, j the candidate's
 * place among that sample's real roots; 0xFFFFFFFF: none), M = matches considered}.
 * The algorithm, exactly (a CPU restatement reproduces every sample: tests/fundamental_ref.py; the kernels' own arithmetic,
 * built for the host, reproduces every output bit: tests/cpp/fundamental_twin.cpp):
 *   1. Considered matches and normalisation: homography step 1, unchanged (the same launch computes them).  As there, a NaN
 *      or infinite coordinate in a considered row leaves the pair without a valid candidate (step 6), and rows that are not
 *      considered are never read.
 *   2. Sampler: sample k takes draws t = 0..63, r = splitmix64(((uint64)(seed + p) << 32) ^ ((uint64)k << 6) ^ t),
 *      pos = ((r >> 32) * M) >> 32, and keeps the first 7 distinct positions (fewer: the sample is invalid).
 *   3. Minimal solver, f32 on the normalised coordinates, using only correctly rounded operations (+ - * /, sqrt, fma) with
 *      fixed iteration counts.  Sampled match i gives the row [u x, u y, u, v x, v y, v, x, y, 1] (a = (x, y), b = (u, v)).
 *      Gauss-Jordan elimination with full pivoting: at each of the 7 steps the pivot is the largest |entry| among the rows and
 *      columns not used yet (the first in row-major order on a tie); the sample is invalid if it is not above 1e-5 times the
 *      first pivot.  Every other row r gets row_r + (-(a_r * (1 / pivot))) * pivot row as fma, its pivot-column entry set to 0.
 *      F1, F2 = the null vectors with 1 in the first, resp. second, unused column and 0 in the other (the rest: -(a * (1 / d))
 *      from each pivot row).  With G = F2, D = F1 - F2 and Cof() the cofactor matrix: det(l F1 + (1 - l) F2) = c3 l^3 + c2 l^2
 *      + c1 l + c0, c0 = det G, c1 = sum Cof(G) .* D, c2 = sum Cof(D) .* G, c3 = det D.  No candidate if a coefficient is not
 *      finite or |c3| <= 2^-20 max(|c0|, |c1|, |c2|) (a vanishing leading coefficient: its root near infinity, F = D, is not
 *      sought).  Otherwise the roots lie in [-R, R], R = 1 + max(|c0|, |c1|, |c2|) / |c3|; the derivative's real roots (the
 *      cancellation-free quadratic formula, clamped to [-R, R]) cut it into three monotone pieces; a piece [lo, hi] holds a
 *      root iff (p(lo) < 0) != (p(hi) < 0), found by 40 bisection steps and then 4 Newton steps (a step that leaves the
 *      bracket is not taken).  Each real root l, in ascending order, is candidate j = 0, 1, 2: G + l D, divided by its largest
 *      |entry|, then taken to pixel coordinates F = Tb^T Fn Ta (invalid if that largest |entry| is not finite and positive,
 *      or a value is not finite).
 *   4. Score (Sampson distance, pixels): with l = F a and l' = F^T b, point i is an inlier iff
 *      (b . l)^2 < threshold^2 (l0^2 + l1^2 + l'0^2 + l'1^2).  The best candidate has the largest count; ties go to the
 *      smallest c.
 *   5. Refit (unless LF_MKD_VERIFY_NO_REFINE): least squares sum (r_i . f)^2 over the current F's inliers in the normalised
 *      coordinates of step 1, with f_c = 1 for c the index of the current normalised F's largest |entry| (F33 is not pinned:
 *      it vanishes for sideways camera motion).  The 8x8 normal equations come from the 36 distinct moments
 *      b~_i b~_j a~_k a~_l accumulated in f64 in a fixed order and are solved by the homography's Cholesky and pivot rule.
 *      Rank 2: F <- F (I - v v^T), v the eigenvector of F^T F of the smallest eigenvalue from 6 sweeps of cyclic Jacobi in f64.
 *      The result, divided by its largest |entry|, is rounded to f32, taken to pixels and rescored as in step 4.  It is kept
 *      if its MSAC cost (an inlier adds its Sampson error, any other considered match threshold^2; summed in f64 in a fixed
 *      order) is not above the current F's.  At most 3 rounds, stopping when the inlier set stops changing.
 *   6. M < 7, or no valid candidate: F all zero, verified all -1, final count 0, stats[2] = 0xFFFFFFFF; status LF_MKD_OK.
 *      That is the outcome whenever every sample's 7 x 9 system is rank deficient: all rows identical, fewer than 7 distinct
 *      matches, all points of one image on a line.  Matches that satisfy one homography (a plane, a camera that only turns)
 *      leave a one-parameter family of F: samples whose last pivot is rounding noise above 1e-5 of the first still give
 *      candidates, and every one of them fits the matches; which is returned carries no information about the scene.
 *   Precision.  Steps 2, 3 and 5 work in the normalised coordinates and do not depend on where the origin is.  Step 4 and
 *   the returned F do: in pixel coordinates F's constant entry is of the order of C^2 times its leading ones for points at a
 *   distance C from the origin, and every f32 rounding of it moves the epipolar lines by about C^2 2^-24 / (image extent)
 *   pixels -- 0.001 px for a 1000 px frame at the origin, a pixel at C = 1e5.  Translate coordinates that far away first.
 *   The threshold's smallest accepted values are below what step 4 resolves: a match whose f32 Sampson numerator does not
 *   round to less than threshold^2 times the denominator is not an inlier, be it one of the sample's own seven.
 * The bits of every output depend on the pair's inputs, seed + p, n_hypotheses, threshold and flags alone: pair p of a
 * batched call equals a single-pair call with seed + p, and a captured call replays to the same bits. */

/* Host pointers, one pair, synchronous. */
int lf_mkd_verify_fundamental(lf_mkd *h, const lf_mkd_keypoint *kps_a, uint64_t na,
                              const lf_mkd_keypoint *kps_b, uint64_t nb, const int32_t *match,
                              uint32_t n_hypotheses, float threshold_px, uint32_t seed, uint32_t flags,
                              float *F, int32_t *verified, uint32_t *stats);

/* Device pointers, n_pairs independent problems in one call, asynchronous on `stream` (NULL: the handle's own); three
 * launches, no host synchronisation, no allocation once the handle's scratch has grown (capturable), as
 * lf_mkd_verify_homography_device. */
int lf_mkd_verify_fundamental_device(lf_mkd *h, const lf_mkd_keypoint *d_kps_a, const uint64_t *d_offsets_a,
                                     const lf_mkd_keypoint *d_kps_b, const uint64_t *d_offsets_b,
                                     const int32_t *d_match, uint32_t n_pairs, uint32_t n_hypotheses,
                                     float threshold_px, uint32_t seed, uint32_t flags,
                                     float *d_F, int32_t *d_verified, uint32_t *d_stats, void *stream);

#define LF_MKD_VERIFY_NO_REFINE 1u   /* report the best RANSAC candidate as is: no least-squares refit (both verifiers) */
#define LF_MKD_MATCH_MUTUAL 1u       /* lf_mkd_match_pairs_device: keep a match only if the other direction agrees */
#define LF_MKD_GUIDE_HOMOGRAPHY 0u   /* lf_mkd_match_guided_pairs_device, kind: d_model holds the pairs' H (b ~ H a) */
#define LF_MKD_GUIDE_FUNDAMENTAL 1u  /* ... the pairs' F (b^T F a = 0) */

/* ---- multi-GPU: the path's ONE collective (BASELINE configs[3]) -------------------------------------------------
 * Keypoint batches shard by image, one process and one handle per GPU, and nothing is exchanged while describing.  The
 * cross-image match stage needs every rank's descriptors on every rank: an all-gather of the descriptor shards over RCCL
 * (xGMI).  The reference has no counterpart (one device, one queue: vulkan/make_a_vulkan.rs:80-115); the Rust crate calls
 * these from LocalFeaturesHip::cross_image_match (bindings/rust/).  librccl is loaded when the first of these functions
 * is called (dlopen: a process that has torch's copy loaded gets that one), so the library itself does not depend on it.
 *
 * lf_mkd_comm_unique_id   rank 0 draws the identifier (ncclGetUniqueId) and ships its LF_MKD_COMM_ID_BYTES to the other
 *                         ranks by whatever channel the application has (a file, a socket, MPI, torch.distributed).
 * lf_mkd_comm_create      every rank, with the same identifier: ncclCommInitRank on the handle's device.  Collective.
 * lf_mkd_allgather_descriptors
 *     d_buf   [sum(counts)][128] f32 on the handle's device: the gathered set, rank r's rows at offset sum(counts[0..r));
 *             this rank's own rows are already in place (a producer that writes its descriptors straight there makes
 *             the gather copy-free on the sending side too).
 *     counts  [n_ranks] descriptors held by every rank (host array; shards may differ in size).
 *     mode    LF_MKD_GATHER_DIRECT: one group of point-to-point transfers (ncclGroupStart .. ncclSend / ncclRecv to and from
 *             every peer .. ncclGroupEnd): xGMI is a full point-to-point mesh, so a rank's n-1 sends leave on n-1 links at
 *             once.  LF_MKD_GATHER_RING: one ncclAllGather (in place; needs equal shards, else DIRECT is used).
 *     Asynchronous on `stream` (NULL: the handle's own).  Collective: every rank calls it with the same counts and mode.
 * lf_mkd_comm_info        RCCL's version code, this communicator's size and rank (any pointer may be NULL). */
#define LF_MKD_COMM_ID_BYTES 128
#define LF_MKD_GATHER_DIRECT 0
#define LF_MKD_GATHER_RING 1
typedef struct lf_mkd_comm lf_mkd_comm;
int lf_mkd_comm_unique_id(uint8_t *id);
int lf_mkd_comm_create(lf_mkd *h, const uint8_t *id, int32_t n_ranks, int32_t rank, lf_mkd_comm **out);
int lf_mkd_comm_destroy(lf_mkd_comm *c);
int lf_mkd_comm_info(const lf_mkd_comm *c, int32_t *rccl_version, int32_t *n_ranks, int32_t *rank);
int lf_mkd_allgather_descriptors(lf_mkd *h, lf_mkd_comm *c, const uint64_t *counts, float *d_buf, int32_t mode,
                                 void *stream);
/* Diagnostics of the gather.
 * lf_mkd_comm_loopback: one group with a send of n_rows rows of 128 f32 from d_src to THIS rank and the matching receive into
 *     d_dst (ncclGroupStart, ncclSend, ncclRecv, ncclGroupEnd; n_rows == 0 posts the empty group) -- through the same binding
 *     and the same posting routine as the DIRECT form, whose loop is empty on a one-rank communicator: what lets one process
 *     check that the point-to-point branch works against the librccl it finds, before a multi-rank job depends on it.
 *     d_src and d_dst are DEVICE arrays that must not overlap.  Asynchronous on `stream` (NULL: the handle's own).
 * lf_mkd_comm_last_form: LF_MKD_GATHER_DIRECT or LF_MKD_GATHER_RING, whichever the communicator's latest
 *     lf_mkd_allgather_descriptors took (RING falls back to DIRECT on unequal shards); -1 before the first gather. */
int lf_mkd_comm_loopback(lf_mkd *h, lf_mkd_comm *c, const float *d_src, float *d_dst, uint64_t n_rows, void *stream);
int lf_mkd_comm_last_form(const lf_mkd_comm *c);

/* The same stage on the reference's own buffer formats, for a caller that keeps the reference's detect graph and host
 * filter and swaps only the extract graph.  Host pointers; synchronous.
 *   extremum_data  ExtremumLocations.data: blocks of block_len (256, mod.rs:279) extrema laid out
 *                  [x * block_len][y * block_len][size * block_len][contrast * block_len] f32
 *                  (common.glsl:45-81 `_coord_idx`, host mirror shaders.rs:257-319), n_extrema entries in all;
 *   indices        FilteredExtrema.indices (common.glsl:83-89): the extrema the host filter kept, n_indices of them.
 * Outputs as KeypointIndices holds them (common.glsl:93-101, shaders.rs:321-353): kp_extremum_index[i] = index of
 * keypoint i's extremum (into extremum_data, i.e. one of the values in `indices`) and kp_orientation[i] in degrees,
 * for *n_out <= max_out keypoints, ordered by position in `indices`, then histogram bin.  keypoints (may be NULL) additionally receives
 * the assembled lf_mkd_keypoint records the describe entry points take. */
int lf_mkd_orient_keypoints_blocked(lf_mkd *h, const float *extremum_data, uint64_t n_extrema, uint32_t block_len,
                                    const uint32_t *indices, uint64_t n_indices, uint32_t *kp_extremum_index,
                                    float *kp_orientation, lf_mkd_keypoint *keypoints, uint64_t max_out,
                                    uint64_t *n_out, uint64_t *n_dropped);

/* Verification tap: copies layer `layer` (0 .. n_scales + 2) of frame 0's a-trous stack to a host
 * buffer of width x height floats, building the stack first if needed. */
int lf_mkd_get_coarse_layer(lf_mkd *h, uint32_t layer, float *out);

/* Verification taps for keypoint mode (device pointers). */
int lf_mkd_sample_patches_device(lf_mkd *h, const lf_mkd_keypoint *d_kps, uint64_t n,
                                 float *d_patches, void *stream);
/* Copies pyramid level `level` ((w>>level) x (h>>level) f32) to a host buffer. */
int lf_mkd_get_pyramid_level(lf_mkd *h, uint32_t level, float *out, uint32_t *w, uint32_t *hgt);
/* The same level as the sampler addresses it: with its apron of *apron texels on every side (48 on EVERY level, level 0 included: size
 * the buffer from the returned *apron, never from a constant), which holds
 * what MirroredRepeat addressing (mod.rs:940-943) would fetch there -- (hgt + 2 apron) rows of (w + 2 apron) floats.
 * Any of out / w / hgt / apron may be NULL. */
int lf_mkd_get_pyramid_level_apron(lf_mkd *h, uint32_t level, float *out, uint32_t *w, uint32_t *hgt, uint32_t *apron);

/* lf_mkd_view_graph_device checks the POSED edges of an edge list against each other and gives the images GLOBAL ROTATIONS:
 * the relative rotations around every triangle of images must compose to the identity, an edge between two views of a
 * repeated structure breaks every triangle it closes, and averaging the relative rotations over the edges that survive gives
 * every image a drift-free rotation.  It reads d_edge_a / d_edge_b uint32 [n_edges], d_R f32 [n_edges][9] and d_pose_stats
 * uint32 [n_edges][4] as lf_mkd_two_view_pose_device wrote them (x_b = R x_a + t, so R_b = R R_a for world-to-camera
 * rotations) and, optionally, the matches' edge layout; it writes what the next calls take.
 *  1 usable      edge e = (a, b) is USABLE iff a < n_images, b < n_images, a != b, d_pose_stats[e][2] != 0xFFFFFFFF,
 *                d_pose_stats[e][0] >= min_front and all nine entries of R are finite.  lf_mkd_select_edges_device's 0xFFFFFFFF
 *                padding, self edges and edges without a pose are ordinary input: not usable.
 *  2 quaternion  a usable edge has the unit quaternion q_e (a -> b; (w, x, y, z), Hamilton product, the rotation of p (x) q
 *                is the rotation of p times that of q) of R by Shepperd's method in f64 (+ - * / and sqrt, no contraction):
 *                the largest of (trace, R00, R11, R22), the lowest index on a tie, says which component comes from the
 *                diagonal (1 + 2 max - trace), the other three are the off-diagonal sums and differences; one normalisation.
 *  3 representative   the lowest-indexed usable edge of an unordered pair {i, j}, whichever way it is stored.  q(x -> y) of a
 *                pair is its representative's quaternion, conjugated if it is stored as (y, x).
 *  4 vote        for a usable edge e = (a, b) and every image c outside {a, b} for which both pairs {b, c} and {c, a} have
 *                representatives: closed += 1, L = q(c -> a) (x) (q(b -> c) (x) q_e), consistent += 1 iff
 *                2 L_w^2 - 1 >= cos(max_loop_deg) (the cosine is formed once by the host, in double; no transcendental runs
 *                on the device).  A duplicate edge votes with its own q_e and the other pairs' representatives.  Integer
 *                counts: no order, run or CU count in them.
 *  5 state       0 not usable; 1 rejected (closed > 0, consistent == 0); 2 unchecked (closed == 0); 3 supported
 *                (consistent > 0).
 *  6 kept        the supported representatives; under LF_MKD_VIEW_GRAPH_USE_UNCHECKED the unchecked representatives too.
 *                (On synthetic rings of 24 .. 64 cameras with 10 .. 15 % wrong edges a wrong edge was never supported, but a
 *                wrong edge that closes no triangle, let into the tree, ruined the rotations in about a quarter of the scenes:
 *                hence the default.)
 *  7 root        `root` if it is an image id; for LF_MKD_VIEW_GRAPH_AUTO_ROOT the image with the most kept incident edges, the
 *                lowest id on a tie, chosen on the device.  It gets the identity and is labelled in round 0.
 *  8 tree        in round r = 1 .. tree_rounds an image without a rotation that has kept edges to images labelled in rounds
 *                < r takes q_i = normalise(q(j -> i) (x) q_j) over the best of them: the state first (larger), then
 *                d_pose_stats[.][0] (larger), then the edge index (lower).  Rounds are level-synchronous.
 *  9 averaging   `iterations` sweeps, double-buffered; every labelled image but the root takes part in each.  The predictions
 *                p = q(j -> i) (x) q_j over its kept edges to labelled images are taken in ascending j, each negated iff
 *                p . q_i < 0, and summed per component in the 4-SLOT canonical order of track triangulation: term k (k = 0,
 *                1, .. in ascending j) is added to slot k mod 4 in ascending k, the slots are combined as (s0 + s2) + (s1 + s3);
 *                the lazy term n q_i (n terms) is added and the result normalised.  n == 0: the value stays.
 * 10 outputs     d_rotations f32 [n_images][9], row-major: the rotation of the final q_i; all zero for an image never
 *                  labelled (the pose arrays' "not registered").
 *                d_edge_stats uint32 [n_edges][4] = {closed, consistent, state, the pair's representative (its own index if
 *                  it is one); {0, 0, 0, 0xFFFFFFFF} if not usable}.
 *                d_edge_residual optional, f32 [n_edges]: for a usable edge with both ends labelled the cosine of the angle
 *                  between R and R_b R_a^T under the final rotations, 2 (q_b . (q_e (x) q_a))^2 - 1 in f64; 2 otherwise (the
 *                  pose call's "none").
 *                d_image_stats uint32 [n_images][4] = {kept incident edges, the round it was labelled in (0 the root,
 *                  0xFFFFFFFF never), its tree edge (0xFFFFFFFF none), rejected incident edges (state 1, duplicates counted)}.
 *                d_match_out optional, with d_edge_offsets_a (uint64 [n_edges + 1]) / ea_capacity and d_match as
 *                  lf_mkd_link_table_device reads them: for every entry of edge e's range (both ends clamped to ea_capacity,
 *                  an inverted range empty) d_match[.] if e is kept and -1 otherwise -- a duplicate of a kept pair is not
 *                  kept, so a pair is linked once.  Entries outside every range are untouched.  It may be d_match (every
 *                  entry is read before it is written, by the same thread); lf_mkd_build_tracks_device takes it as d_match.
 *                d_counts uint32 [8] = {usable, supported, rejected, unchecked, kept, images labelled, root, 0}.
 * 11 degenerate  n_edges == 0 with n_images > 0: zero rotations except that a given root gets the identity (its round is 0);
 *                  nothing is labelled under LF_MKD_VIEW_GRAPH_AUTO_ROOT; all eight counts are 0.
 *                n_images == 0: LF_MKD_OK, nothing is written.  tree_rounds == 0: only the root is labelled.
 * Device form: a table uint32 [n_images][n_images] of representatives in the handle's scratch (zeroed by a kernel, filled by
 * an integer atomic min), the quaternions as f64 beside it; a wave per edge votes over two rows of it, a wave per image walks
 * its row for the tree and the sweeps.  No floating-point atomic, no workgroup waits for another, nothing is read back.
 * Launches (lf_mkd_view_graph_plan's `launches`): 3 + tree_rounds + iterations (zero, root, the rounds, the sweeps, final),
 * + 2 with n_edges > 0 (edges, vote), + 1 more with the match arrays; none for n_images == 0.  Asynchronous on `stream`
 * (NULL: the handle's own); the scratch belongs to the handle and only grows, so a warmed-up call is capturable in a hipGraph.
 * Calls of one handle are stream-ordered.  d_image_stats and d_edge_stats also carry the call's state between its launches.
 * LF_MKD_ERR_BAD_ARG ("view_graph_device: "), before any device is touched: with n_images > 0 a null d_rotations,
 * d_image_stats or d_counts, and with n_edges > 0 too a null d_edge_a, d_edge_b, d_R, d_pose_stats or d_edge_stats; only part
 * of d_edge_offsets_a, d_match, d_match_out; unknown flags; max_loop_deg outside [0, 180] or a NaN; a root at or beyond
 * n_images other than LF_MKD_VIEW_GRAPH_AUTO_ROOT; tree_rounds or iterations above LF_MKD_VIEW_GRAPH_MAX_ROUNDS; n_images^2
 * above 2^31 - 1; n_edges above 2^31 - 1; d_edge_offsets_a not 8-byte or any other array not 4-byte aligned; ea_capacity
 * above 2^31 - 1. */
#define LF_MKD_VIEW_GRAPH_USE_UNCHECKED (1u)        /* keep the representatives that close no triangle too */
#define LF_MKD_VIEW_GRAPH_AUTO_ROOT (0xFFFFFFFFu)   /* `root`: the image with the most kept incident edges */
#define LF_MKD_VIEW_GRAPH_MAX_ROUNDS (4096u)        /* the largest tree_rounds and the largest iterations */
#define LF_MKD_VIEW_GRAPH_FORM_TABLE (0u)           /* the plan's form: the dense table of representatives */
/* Host only: the launches and the scratch of lf_mkd_view_graph_device for these sizes (with_match != 0: the match arrays are
 * given), and its form (LF_MKD_VIEW_GRAPH_FORM_TABLE, the only one).  Any output may be NULL.  LF_MKD_ERR_BAD_ARG
 * ("view_graph_plan: "): the sizes, rounds and flags the device call refuses. */
int lf_mkd_view_graph_plan(uint32_t n_images, uint32_t n_edges, uint32_t tree_rounds, uint32_t iterations, uint32_t flags,
                           uint32_t with_match, uint32_t *launches, uint64_t *scratch_bytes, uint32_t *form);
int lf_mkd_view_graph_device(lf_mkd *h, const uint32_t *d_edge_a, const uint32_t *d_edge_b, uint32_t n_edges, const float *d_R,
                             const uint32_t *d_pose_stats, uint32_t n_images, float max_loop_deg, uint32_t min_front, uint32_t root,
                             uint32_t tree_rounds, uint32_t iterations, uint32_t flags, const uint64_t *d_edge_offsets_a,
                             uint64_t ea_capacity, const int32_t *d_match, int32_t *d_match_out, float *d_rotations,
                             uint32_t *d_edge_stats, float *d_edge_residual, uint32_t *d_image_stats, uint32_t *d_counts,
                             void *stream);
/* The host form: host arrays in and out, staged through the handle; synchronous.  match has n_entries entries and is filtered
 * on its staged copy, so match_out (which may be match) gets match's value in every entry outside the edges' ranges.
 * LF_MKD_ERR_BAD_ARG ("view_graph: ") as above, without the alignment rules. */
int lf_mkd_view_graph(lf_mkd *h, const uint32_t *edge_a, const uint32_t *edge_b, uint32_t n_edges, const float *R,
                      const uint32_t *pose_stats, uint32_t n_images, float max_loop_deg, uint32_t min_front, uint32_t root,
                      uint32_t tree_rounds, uint32_t iterations, uint32_t flags, const uint64_t *edge_offsets_a, uint64_t n_entries,
                      const int32_t *match, int32_t *match_out, float *rotations, uint32_t *edge_stats, float *edge_residual,
                      uint32_t *image_stats, uint32_t *counts);

/* lf_mkd_tree_poses_device gives every image the view graph labelled an INITIAL POSE: the rotation the view graph gave it and
 * a centre one unit step from its tree parent's, along the direction of the tree edge's translation.  It reads d_edge_a /
 * d_edge_b uint32 [n_edges] and d_t f32 [n_edges][3] as lf_mkd_two_view_pose_device wrote them (x_b = R x_a + t, so c_b - c_a
 * is parallel to 0 - R_b^T t), and d_rotations f32 [n_images][9] and d_image_stats uint32 [n_images][4] as
 * lf_mkd_view_graph_device wrote them (word 1 the round, word 2 the tree edge).  It writes d_poses f32 [n_images][12] (R
 * row-major, then t; world to camera), the array lf_mkd_global_positions_device starts from.
 *  1 chain     image i's chain is i, its tree edge's other end, that image's, .. up to an image of round 0 (the root).  The
 *              chain BREAKS at an image whose round is 0xFFFFFFFF or whose rotation is all zero, at a tree edge at or beyond
 *              n_edges, at an edge with an end at or beyond n_images, with equal ends or that the image is no end of, at a
 *              non-finite t or rotation of the edge's b, at a step of no length, and after max_depth steps without a root.
 *  2 step      of a tree edge (a, b): d = 0 - R_b^T t under the view graph's R_b, u = d / sqrt(d.d), f64 (+ - * / and sqrt,
 *              no contraction).  The image at end b stands at its parent's centre + u, the image at end a at its parent's - u.
 *  3 centre    the root's is 0; every other image's is the sum of its chain's steps from the root down, in that order, so
 *              c_i = c_parent +/- u to the bit and every word depends on the image's own chain alone.
 *  4 output    a broken chain: the all-zero row ("not registered").  Otherwise R as given and t = 0 - R c, rounded once to
 *              f32 (the root: [R | 0]).
 * One launch, a thread per image, no scratch; a thread takes its chain 32 images at a time from the root's end and walks up
 * to each run again, so an image at depth d costs d steps and d^2 / 64 reads of a parent.  Asynchronous on `stream` (NULL: the handle's own); capturable.  n_images == 0: LF_MKD_OK, nothing written.
 * LF_MKD_ERR_BAD_ARG ("tree_poses_device: "), before any device is touched: with n_images > 0 a null d_rotations,
 * d_image_stats or d_poses, and with n_edges > 0 too a null d_edge_a, d_edge_b or d_t; max_depth above
 * LF_MKD_VIEW_GRAPH_MAX_ROUNDS; an array not 4-byte aligned; n_images or n_edges above 2^31 - 1. */
int lf_mkd_tree_poses_device(lf_mkd *h, const uint32_t *d_edge_a, const uint32_t *d_edge_b, const float *d_t, uint32_t n_edges,
                             const float *d_rotations, const uint32_t *d_image_stats, uint32_t n_images, uint32_t max_depth,
                             float *d_poses, void *stream);
/* The host form: host arrays in and out, staged through the handle; synchronous.  LF_MKD_ERR_BAD_ARG ("tree_poses: ") as
 * above, without the alignment rule. */
int lf_mkd_tree_poses(lf_mkd *h, const uint32_t *edge_a, const uint32_t *edge_b, const float *t, uint32_t n_edges,
                      const float *rotations, const uint32_t *image_stats, uint32_t n_images, uint32_t max_depth, float *poses);

/* lf_mkd_global_positions_device finds ALL CAMERA CENTRES AND ALL TRACK POINTS AT ONCE under held rotations: with R_i known an
 * observation constrains X_k - c_i to a known world ray, so each adds a linear term in the two unknown positions, and
 * alternating the points' and the cameras' 3x3 solves under robust weights converges without an initial pair and without
 * resection rounds.  It reads the keypoints, the images' row ranges, the track table, the intrinsics and the poses as
 * lf_mkd_bundle_adjust_device reads them, and d_row_track int32 [n_rows_total] as lf_mkd_resect_cameras_device reads it; the
 * rotations of d_poses are held and 0 - R^T t is the initial centre (lf_mkd_tree_poses_device writes such an array).  T and O
 * are d_table_counts[0] and [1] clamped to the capacities; ranges are clamped as in the sibling calls.
 *  1 registered  image i takes part iff tri-usable: finite intrinsics with fx, fy > 0, twelve finite pose values, R not all zero.
 *  2 usable      position p of the observation arrays is USABLE iff 0 <= d_obs_row[p] < n_rows_total, d_obs_image[p] is a
 *                registered image and the row's x and y are finite.  A ROW r of registered image i (in its clamped range)
 *                is usable iff 0 <= d_row_track[r] < T and its x and y are finite.  (The two agree on a table and a row map
 *                from the same lf_mkd_track_table_device call.)  Its ray is v = R_i^T f / |f|, f = ((x - cx) / fx,
 *                (y - cy) / fy, 1), as track triangulation forms it; its projector is P = I - v v^T.
 *  3 weight      of an observation against a point X and a centre c, r = X - c: 1 under unit weights.  Under robust
 *                weights 0 if v . r <= 0, r is zero or anything is not finite; else s0 / s if s = sqrt(|P r|^2 / |r|^2) > s0
 *                and 1 otherwise, s0 = sin(robust_deg) formed once by the host in double.  Sweep s = 0, 1, .. has unit
 *                weights iff s < warm.
 *  4 point step  for track k < T: A = sum w P, g = sum w P c_i over its usable positions in table order, per component in
 *                the 4-SLOT canonical order of track triangulation (position lo + j in slot j mod 4, ascending; (s0 + s2) +
 *                (s1 + s3)); w against the point's previous value, and 1 if the point was unsolved in the previous sweep
 *                (every point before the first).  If at least min_obs positions have w > 0 and the cofactor solve of track
 *                triangulation accepts A with a finite result, X_k = A^-1 g and the point is SOLVED; otherwise it is
 *                unsolved for this sweep, keeps its value, and its observations add nothing to the camera step.
 *  5 camera step for registered image i: A = sum w P, g = sum w P X_k over its usable rows in solved tracks in ascending
 *                row order, per component in the 256-SLOT canonical order of resection (row lo + j in slot j mod 256; the
 *                butterfly within each 64 slots, then ((w0 + w1) + w2) + w3); w against the new points and the camera's
 *                previous centre.  Solved under the same two conditions; otherwise HELD: it keeps its centre and the sweep
 *                counts it.
 *  6 gauge       before the first sweep and after every sweep, over the registered cameras (camera i in slot i mod 256 of
 *                the 256-slot order): the mean m of their centres, rho = sqrt(sum |c - m|^2 / n); centres and all T points
 *                become (. - m) / rho.  If there is no registered camera or m or rho is not finite and positive, nothing is
 *                rescaled and d_counts[5] counts it.  The output lives in this gauge: centroid 0, rms radius 1.  (The gauge
 *                before the first sweep makes the call invariant to a similarity of the input's centres.)
 *  7 final       the final weights are against the final points and centres, under the last sweep's rule (unit without a
 *                sweep); an observation of an unsolved track has none.
 *  8 outputs     d_poses_out f32 [n_images][12], may be d_poses: R as given and t = 0 - R c rounded to f32; the zero row
 *                  for an image that is not registered.
 *                d_points_out optional, f32 [track_capacity][4] = {X, Y, Z, c} for the tracks below T, c the smallest
 *                  cosine between the ray of the track's first position of final weight > 0 and each later such one (2 if
 *                  there is none); {0, 0, 0, 2} for an unsolved track.  These points are what the sweeps minimised; the
 *                  canonical points for the bundle still come from lf_mkd_triangulate_tracks_device under d_poses_out.
 *                d_obs_state optional, uint32 [obs_capacity], for the positions inside the ranges of the tracks below T: 0
 *                  not usable, 1 usable, 2 final weight at least 1/2.  Other entries are untouched.
 *                d_image_stats uint32 [n_images][4] = {usable rows in solved tracks, those of final weight at least 1/2,
 *                  sweeps in which it was held, reason of its last step: 0 solved (or no sweep), 1 not registered, 2 fewer
 *                  than min_obs weighted rows, 3 singular}.
 *                d_trace optional, f64 [sweeps][4] = {the weighted cost sum w |P r|^2 after the sweep's gauge under the
 *                  sweep's rule over the usable positions p < O whose row's track is solved, position p in slot p mod 256
 *                  of the 256-slot order; the positions with w > 0; cameras held; points unsolved}.
 *                d_counts uint32 [8] = {registered images, solved points, usable rows in solved tracks, those of final
 *                  weight at least 1/2, cameras held in the last sweep, gauge steps that did not rescale, T, sweeps}.
 *  9 degenerate  sweeps == 0: the input's centres in the output gauge, every point unsolved.  n_images == 0: LF_MKD_OK,
 *                  nothing is written.
 * Device form: launches (lf_mkd_global_positions_plan's `launches`) 4 + 3 sweeps: init, gauge, then per sweep points (4 lanes
 * own a track), cameras (a workgroup owns an image) and gauge (ONE workgroup), final images, final tracks; none for n_images
 * == 0.  The gauge rescales the centres itself and hands m and rho on: the points are rescaled by whoever reads them next, the
 * same operations on the same values.  A single image that owns every row is walked by one workgroup, a single track with
 * every observation by 4 lanes, AND WITH A TRACE THE GAUGE'S COST PASS WALKS ALL O OBSERVATIONS IN ONE WORKGROUP: pass no
 * d_trace where time matters.  No floating-point atomic, no workgroup waits for another, nothing is read back.
 * Asynchronous on `stream` (NULL: the handle's own); the scratch belongs to the handle and only grows, so a warmed-up call is
 * capturable in a hipGraph.  Calls of one handle are stream-ordered.
 * LF_MKD_ERR_BAD_ARG ("global_positions_device: "), before any device is touched: with n_images > 0 a null d_image_offsets,
 * d_table_counts, d_intrinsics, d_poses, d_poses_out, d_image_stats or d_counts; with track_capacity > 0 too a null
 * d_track_offsets, and with obs_capacity > 0 too a null d_obs_row or d_obs_image; with n_images > 0 and n_rows_total > 0 a null
 * d_kps or d_row_track; flags other than 0; sweeps above LF_MKD_GLOBAL_POSITIONS_MAX_SWEEPS; robust_deg outside (0, 90] or a
 * NaN; min_obs below 2; d_image_offsets, d_track_offsets or d_trace not 8-byte or any other array not 4-byte aligned; a total
 * or a capacity above 2^31 - 1. */
#define LF_MKD_GLOBAL_POSITIONS_MAX_SWEEPS (4096u)  /* the largest sweeps */
/* Host only: the launches and the scratch of lf_mkd_global_positions_device for these sizes.  Either output may be NULL.
 * LF_MKD_ERR_BAD_ARG ("global_positions_plan: "): the sweeps and sizes the device call refuses. */
int lf_mkd_global_positions_plan(uint32_t n_images, uint64_t track_capacity, uint32_t sweeps, uint32_t *launches,
                                 uint64_t *scratch_bytes);
int lf_mkd_global_positions_device(lf_mkd *h, const lf_mkd_keypoint *d_kps, const uint64_t *d_image_offsets, uint32_t n_images,
                                   uint64_t n_rows_total, const uint64_t *d_track_offsets, uint64_t track_capacity,
                                   const int32_t *d_obs_row, const uint32_t *d_obs_image, uint64_t obs_capacity,
                                   const uint32_t *d_table_counts, const int32_t *d_row_track, const float *d_intrinsics,
                                   const float *d_poses, uint32_t sweeps, uint32_t warm, float robust_deg, uint32_t min_obs,
                                   uint32_t flags, float *d_poses_out, float *d_points_out, uint32_t *d_obs_state,
                                   uint32_t *d_image_stats, double *d_trace, uint32_t *d_counts, void *stream);
/* The host form: host arrays in and out, staged through the handle, with n_tracks and n_obs as the table's counts;
 * synchronous.  obs_state's entries outside every track's range come back 0.  LF_MKD_ERR_BAD_ARG ("global_positions: ") as
 * above, without the alignment rules. */
int lf_mkd_global_positions(lf_mkd *h, const lf_mkd_keypoint *kps, const uint64_t *image_offsets, uint32_t n_images,
                            uint64_t n_rows_total, const uint64_t *track_offsets, uint64_t n_tracks, const int32_t *obs_row,
                            const uint32_t *obs_image, uint64_t n_obs, const int32_t *row_track, const float *intrinsics,
                            const float *poses, uint32_t sweeps, uint32_t warm, float robust_deg, uint32_t min_obs, uint32_t flags,
                            float *poses_out, float *points_out, uint32_t *obs_state, uint32_t *image_stats, double *trace,
                            uint32_t *counts);

/* Host-only verification tap: the constants upload_constant_data (mod.rs:1587-1713) would place in
 * ConstantData (common.glsl:34-40), as this library builds them.  Any output pointer may be NULL.
 * gradient_angle[1024], embedding_polar[25*1024], embedding_cartesian[9*1024], w_t[128*238].
 * Needs no device. */
int lf_mkd_build_constants(const float *mean, const float *eigvals, const float *eigvecs,
                           float *gradient_angle, float *embedding_polar,
                           float *embedding_cartesian, float *w_t);

/* With LF_MKD_FLAG_KERNEL_TIMING: waits for the recorded launches, returns the summed device time
 * (ms) of the describe kernel (pool_ms; whiten_ms is 0 since the whitening stage was fused into it)
 * and the number of batches since the previous call, then resets the sums.  Any output pointer may
 * be NULL.  Covers the describe launches the patch and keypoint entry points make (and a stage-by-stage
 * lf_mkd_detect); a REPLAYED lf_mkd_detect / lf_mkd_stream_frame launches its describe node inside the
 * hipGraph, without events: lf_mkd_detect_times covers those. */
int lf_mkd_kernel_times(lf_mkd *h, double *pool_ms, double *whiten_ms, uint64_t *launches);

/* With LF_MKD_FLAG_KERNEL_TIMING: where the handle's latest lf_mkd_detect / lf_mkd_detect_u8 call spent its time -- the upload of
 * the frame and the recorded pipeline (HIP events on the handle's stream around each), and the wall time from the pipeline's
 * end to the return (the copy of the results to the caller's arrays).  Any output pointer may be NULL. */
int lf_mkd_detect_times(lf_mkd *h, double *upload_ms, double *pipeline_ms, double *readback_ms);

/* With LF_MKD_FLAG_KERNEL_TIMING: the shader clock the chip sustained during the handle's latest describe launch, from
 * stamps workgroup 0 of the kernel leaves on entry and exit (shader-clock counter / constant 100 MHz counter), and that
 * workgroup's lifetime in ms.  The chip lowers its clock under load, box by box: this is what makes two boxes' figures
 * comparable.  Waits for `stream` (NULL: the handle's own).  Either output pointer may be NULL. */
int lf_mkd_kernel_clock(lf_mkd *h, void *stream, double *shader_mhz, double *kernel_ms);

/* Diagnostic of lf_mkd_detect / lf_mkd_detect_u8 (host state only, no device work): how many recorded pipelines the handle holds
 * at the moment (at most 8), how many of them upload their frame in pieces, and how many distinct requests it remembers having
 * seen (at most 64; a request is recorded on its second sighting).  Any output pointer may be NULL. */
int lf_mkd_detect_recordings(const lf_mkd *h, uint32_t *n_recordings, uint32_t *n_banded, uint32_t *n_sightings);

/* Blocks until everything enqueued on the handle's own stream has finished. */
int lf_mkd_synchronize(lf_mkd *h);

/* Library identification: "lf_mkd <version> gfx950". */
const char *lf_mkd_version(void);

#ifdef __cplusplus
}
#endif
#endif /* LF_MKD_H */
