// C ABI of the MKD path (include/lf_mkd.h): handle management, batching, host<->device staging; describe, the pyramid,
// orientation, detection and the recorded pipelines.  The matchers, the tables and the geometry are lf_mkd_match.cpp,
// lf_mkd_tables.cpp and lf_mkd_geometry.cpp, over the same handle (lf_mkd_handle.h).
// Product code: it never touches oracle/; without a HIP device every entry point fails loudly.
#include "../../include/lf_mkd.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <utility>
#include <vector>

#include "lf_mkd_handle.h"
#include "mkd_consts.hpp"
#include "mkd_device.h"

using namespace lfmkd;

namespace lfmkd {
thread_local std::string g_create_error;
}  // namespace lfmkd

namespace {

template <typename T>
hipError_t upload(HipArray<T> &dst, const std::vector<T> &src) {
    hipError_t e = dst.allocate(src.size());
    if (e != hipSuccess) return e;
    return hipMemcpy(dst, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice);
}

long pyramid_levels(uint32_t w, uint32_t h) {  // mod.rs:271-277,372-373
    return std::lround(std::ceil(std::log2(float(std::min(w, h)))));
}

// returns the floats one frame's pyramid occupies (every level with its mirrored apron: mkd_device.h)
long describe_pyramid(uint32_t w, uint32_t h, PyramidDesc &pd) {
    pd.levels = int(std::min<long>(std::max<long>(pyramid_levels(w, h), 1), kMaxPyrLevels));
    long off = 0;
    for (int l = 0; l < pd.levels; ++l) {
        pd.w[l] = std::max<int>(int(w >> l), 1);
        pd.h[l] = std::max<int>(int(h >> l), 1);
        pd.apron[l] = kPyrApron;
        pd.pitch[l] = pd.w[l] + 2 * pd.apron[l];
        pd.offset[l] = off + long(pd.apron[l]) * pd.pitch[l] + pd.apron[l];
        off += long(pd.pitch[l]) * (pd.h[l] + 2 * pd.apron[l]);
    }
    return (off + 63) / 64 * 64;   // frames 256 bytes apart at least: level 0 of every frame starts 16-byte aligned (pyr_swt_staged)
}

long pyramid_floats(uint32_t w, uint32_t h) {
    PyramidDesc pd{};
    return describe_pyramid(w, h, pd);
}

int create_impl(const lf_mkd_params *params, const PcaModel &pca, lf_mkd **out) {
    if (!params || !out) return LF_MKD_ERR_BAD_ARG;
    *out = nullptr;
    // the model first: a bad model is the caller's error whatever the machine (and is reported without a device)
    HostConsts hc;
    if (const std::string e = build_host_consts(pca, hc); !e.empty()) {
        g_create_error = e;
        return LF_MKD_ERR_BAD_ARG;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || params->device < 0 || params->device >= ndev) {
        g_create_error = "no HIP device " + std::to_string(params->device) + " (devices visible: " +
                         std::to_string(ndev) + ")";
        return LF_MKD_ERR_NO_DEVICE;
    }
    lf_mkd *h = new (std::nothrow) lf_mkd;
    if (!h) return LF_MKD_ERR_BAD_ARG;
    h->params = *params;
    if (h->params.patch_scale_factor == 0.f) h->params.patch_scale_factor = 24.f;  // lib.rs:46
    if (h->params.pool_mode == LF_MKD_POOL_DEFAULT) h->params.pool_mode = LF_MKD_POOL_F16X3;
    if (h->params.pool_mode != LF_MKD_POOL_F16X3 && h->params.pool_mode != LF_MKD_POOL_F32 &&
        h->params.pool_mode != LF_MKD_POOL_F16_FP6) {
        g_create_error = "pool_mode must be LF_MKD_POOL_DEFAULT, LF_MKD_POOL_F16X3, LF_MKD_POOL_F32 or LF_MKD_POOL_F16_FP6";
        delete h;
        return LF_MKD_ERR_BAD_ARG;
    }
    if (h->params.angle_mode < LF_MKD_ANGLE_SHADER || h->params.angle_mode > LF_MKD_ANGLE_EXACT_ZERO) {
        g_create_error = "angle_mode must be one of lf_mkd_angle_mode";
        delete h;
        return LF_MKD_ERR_BAD_ARG;
    }
    const uint64_t mf = params->max_features ? params->max_features : 2000;        // lib.rs:69
    h->n_layers = int(params->n_scales ? params->n_scales : 4) + 3;                // lib.rs:70, mod.rs:1093
    if (h->n_layers - 1 > 8) {   // the extremum scan keeps at most 8 DoG layers of a tile in LDS
        g_create_error = "n_scales must not exceed 6";
        delete h;
        return LF_MKD_ERR_BAD_ARG;
    }
    h->max_extrema = 256 * ((uint64_t(params->max_blobs ? params->max_blobs : 8000) + 255) / 256);  // mod.rs:279-286
    if (const char *e = getenv("LF_MKD_DETECT_RECORD_AFTER")) h->record_after = uint64_t(std::max(0, atoi(e)));
    h->batch = (mf + 63) / 64 * 64;
    auto bail = [&](int code) {
        g_create_error = h->err;
        lf_mkd_destroy(h);
        return code;
    };
#define LF_CREATE_HIP(call)                                                   \
    do {                                                                      \
        hipError_t e_ = (call);                                               \
        if (e_ != hipSuccess) {                                               \
            h->err = std::string(#call) + ": " + hipGetErrorString(e_);       \
            return bail(LF_MKD_ERR_HIP);                                      \
        }                                                                     \
    } while (0)
    lfmkd::DeviceScope scope_;
    LF_CREATE_HIP(scope_.enter(params->device));
    LF_CREATE_HIP(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    {
        hipDeviceProp_t prop;
        LF_CREATE_HIP(hipGetDeviceProperties(&prop, params->device));
        h->num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    }
    auto &c = h->consts;
    LF_CREATE_HIP(upload(c.colmap, hc.colmap));
    LF_CREATE_HIP(upload(c.pool_b_f32, hc.pool_b_f32));
    LF_CREATE_HIP(upload(c.pool_b_f16, hc.pool_b_f16));
    if (h->params.pool_mode == LF_MKD_POOL_F16_FP6) {   // the unfolded row form's own tables
        LF_CREATE_HIP(upload(c.pool_b_fp6, hc.pool_b_fp6));
        LF_CREATE_HIP(upload(c.colmap_unfolded, hc.colmap_unfolded));
        LF_CREATE_HIP(upload(c.white_a_f16_unfolded, hc.white_a_f16_unfolded));
    }
    LF_CREATE_HIP(upload(c.white_a_f16, hc.white_a_f16));
    LF_CREATE_HIP(upload(c.white_a_f32, hc.white_a_f32));
    LF_CREATE_HIP(upload(c.white_bias, hc.white_bias));
    {
        std::vector<float> oc(hc.odd_cart_fx, hc.odd_cart_fx + 16);
        oc.insert(oc.end(), &hc.odd_cart_gy[0][0], &hc.odd_cart_gy[0][0] + 32 * 4);
        LF_CREATE_HIP(upload(c.odd_cart, oc));
    }
    h->dc = DeviceConsts{c.colmap, c.pool_b_f32, c.pool_b_f16, c.white_a_f16, c.white_a_f32, c.colmap_unfolded, c.pool_b_fp6,
                         c.white_a_f16_unfolded, c.white_bias, c.odd_cart};
    // (the staging buffers of the host-pointer and keypoint entry points -- 4.6 KiB per descriptor of the internal batch --
    // are allocated on first use: a caller of the device-pointer patch API never needs them)
    LF_CREATE_HIP(h->d_totals.allocate(8));
    LF_CREATE_HIP(h->d_claims.allocate(lf_mkd::kClaimSlots * lf_mkd::kClaimStride));
    if (h->params.flags & LF_MKD_FLAG_KERNEL_TIMING) {
        LF_CREATE_HIP(h->d_clk.allocate(4));
        LF_CREATE_HIP(hipMemset(h->d_clk, 0, 4 * sizeof(unsigned long long)));
    }
    if (params->max_image_width && params->max_image_height) {
        // the sampler addresses a pyramid level with 32-bit byte offsets from its first texel
        if ((uint64_t(params->max_image_width) + 2 * kPyrApron) * (uint64_t(params->max_image_height) + 2 * kPyrApron) >= (1ull << 30) ||
            params->max_image_width >= (1u << 20) || params->max_image_height >= (1u << 20)) {
            h->err = "max_image_width x max_image_height (with the pyramid's apron of 48 texels a side) must stay below 2^30 pixels";
            return bail(LF_MKD_ERR_BAD_ARG);
        }
        h->max_frames = params->max_frames ? params->max_frames : 1;
        const size_t px = size_t(params->max_image_width) * params->max_image_height * h->max_frames;
        h->pyr_stride = pyramid_floats(params->max_image_width, params->max_image_height);
        h->layer_stride = long(params->max_image_width) * params->max_image_height;
        h->coarse_stride = h->layer_stride * (h->n_layers - 1);
        LF_CREATE_HIP(h->d_image.allocate(px));
        LF_CREATE_HIP(h->d_tmp_a.allocate(px));
        LF_CREATE_HIP(h->d_tmp_b.allocate(px));
        LF_CREATE_HIP(h->d_pyr.allocate(size_t(h->pyr_stride) * h->max_frames));
        if (h->params.pool_mode == LF_MKD_POOL_F16X3 && !(h->params.flags & LF_MKD_FLAG_UNFUSED_KEYPOINTS)) {
            LF_CREATE_HIP(h->d_kp_xchg.allocate(kp_split_exchange_bytes(h->num_cus) / sizeof(float)));
            LF_CREATE_HIP(h->d_kp_words.allocate(kp_split_counter_words(h->num_cus)));
            LF_CREATE_HIP(hipMemset(h->d_kp_words, 0, kp_split_counter_words(h->num_cus) * 4));
        }
    }
#undef LF_CREATE_HIP
    *out = h;
    return LF_MKD_OK;
}

// staging for one internal batch: sampled / uploaded patches; descriptors on their way to the host and uploaded keypoints
int ensure_patch_staging(lf_mkd *h) { return grow(h, h->d_patches, h->batch * kPx); }
int ensure_io_staging(lf_mkd *h) {
    if (int rc = grow(h, h->d_out, h->batch * kOut)) return rc;
    return grow(h, h->d_kps, h->batch * 5);
}
int ensure_staging(lf_mkd *h) {
    if (int rc = ensure_patch_staging(h)) return rc;
    return ensure_io_staging(h);
}

// LF_MKD_FLAG_KERNEL_TIMING: an event on the launch stream before and after every describe launch
int mark(lf_mkd *h, hipStream_t s) {
    if (!(h->params.flags & LF_MKD_FLAG_KERNEL_TIMING)) return LF_MKD_OK;
    hipEvent_t e;
    if (!h->ev_free.empty()) {
        e = h->ev_free.back();
        h->ev_free.pop_back();
    } else {
        LF_HIP(h, hipEventCreate(&e));
    }
    h->ev_pending.push_back(e);
    LF_HIP(h, hipEventRecord(e, s));
    return LF_MKD_OK;
}

int ensure_side_stream(lf_mkd *h, size_t events) {
    if (!h->side_stream) LF_HIP(h, hipStreamCreateWithFlags(&h->side_stream, hipStreamNonBlocking));
    while (h->side_events.size() < events) {
        hipEvent_t e;
        LF_HIP(h, hipEventCreateWithFlags(&e, hipEventDisableTiming));
        h->side_events.push_back(e);
    }
    return LF_MKD_OK;
}

// patches of one batch, already resident on the device -> descriptors (or the un-whitened 238-D vectors)
int run_batch(lf_mkd *h, const float *d_patches, uint64_t n, float *d_out, float *d_raw, hipStream_t s, int waves = 0) {
    if (int rc = mark(h, s)) return rc;
    launch_describe(d_patches, long(n), nullptr, h->dc, h->params.angle_mode, h->params.pool_mode, d_out ? d_out : h->d_out,
                    d_raw, h->num_cus, s, waves, h->d_clk, h->next_claim());
    LF_HIP(h, hipGetLastError());
    if (int rc = mark(h, s)) return rc;
    return LF_MKD_OK;
}

// Keypoints resident on the device -> descriptors.  The product form is ONE launch: producer waves of the describe kernel
// sample the patches into its LDS ring (f16x3 pooling).  The f32 verification mode and LF_MKD_FLAG_UNFUSED_KEYPOINTS take
// the two-launch form through the staging patches in HBM, an internal batch at a time; same sampling arithmetic, same bits.
bool fused_keypoints(const lf_mkd *h) {
    return h->params.pool_mode == LF_MKD_POOL_F16X3 && !(h->params.flags & LF_MKD_FLAG_UNFUSED_KEYPOINTS);
}
int describe_keypoints_on_device(lf_mkd *h, const float *d_kps, const uint32_t *d_frame_of, uint64_t n, float *d_out,
                                 hipStream_t s, uint64_t form_n = 0) {
    if (fused_keypoints(h)) {
        if (int rc = mark(h, s)) return rc;
        launch_describe_keypoints(h->d_pyr, h->pyr_stride, h->pd, d_kps, d_frame_of, h->n_frames, long(n), nullptr,
                                  h->params.patch_scale_factor, h->dc, h->params.angle_mode, d_out, h->num_cus, s, h->d_clk,
                                  h->d_kp_xchg, h->d_kp_words, long(form_n));
        LF_HIP(h, hipGetLastError());
        return mark(h, s);
    }
    if (int rc = ensure_patch_staging(h)) return rc;
    for (uint64_t off = 0; off < n; off += h->batch) {
        const uint64_t m = std::min<uint64_t>(h->batch, n - off);
        launch_sample_patches(h->d_pyr, h->pyr_stride, h->pd, d_kps + off * 5, d_frame_of ? d_frame_of + off : nullptr,
                              h->n_frames, long(m), nullptr, h->params.patch_scale_factor, h->d_patches, s);
        LF_HIP(h, hipGetLastError());
        if (int rc = run_batch(h, h->d_patches, m, d_out + off * kOut, nullptr, s)) return rc;
    }
    return LF_MKD_OK;
}

// the a-trous stack's store: max_frames frames of the maximum size, allocated on first use
int ensure_coarse_store(lf_mkd *h) { return grow(h, h->d_coarse, size_t(h->coarse_stride) * h->max_frames); }

// Extends the loaded frames' level 0 into the a-trous stack (once per set_image*), allocating it on first use.
int ensure_coarse_stack(lf_mkd *h, hipStream_t s) {
    if (h->coarse_valid) return LF_MKD_OK;
    if (int rc = ensure_coarse_store(h)) return rc;
    launch_build_coarse_stack(h->d_pyr + h->pd.offset[0], h->pyr_stride, h->pd.pitch[0], h->d_coarse, h->coarse_stride, h->layer_stride,
                              h->d_tmp_a, h->n_layers, h->coarse_l1_valid ? 1 : 0, h->pd.w[0], h->pd.h[0],
                              int(h->n_frames), s);
    LF_HIP(h, hipGetLastError());
    h->coarse_valid = true;
    return LF_MKD_OK;
}

// the orientation scratch for n extrema (sized for max(n, batch) of them) and, with staging, the rows of max_out keypoints
int ensure_orient_scratch(lf_mkd *h, uint64_t n, bool staging, uint64_t max_out) {
    const uint64_t cap = std::max<uint64_t>(n, h->batch);
    if (int rc = grow(h, h->d_extrema, cap)) return rc;
    if (int rc = grow(h, h->d_angles, cap * LF_MKD_MAX_ANGLES_PER_EXTREMUM)) return rc;
    if (int rc = grow(h, h->d_counts, cap)) return rc;
    if (int rc = grow(h, h->d_orient_sums, cap / 1024 + 2)) return rc;
    if (!staging) return LF_MKD_OK;
    if (int rc = grow(h, h->d_kps_out, max_out)) return rc;
    return grow(h, h->d_det_desc, max_out * kOut);
}

constexpr int kBorder = 5;                  // mod.rs:405
constexpr float kContrastThreshold = 0.035f; // mod.rs:76
constexpr int kSkipLayers = 0;              // mod.rs:398

// the top-n selection's count per frame
int ensure_sel_count(lf_mkd *h) { return grow(h, h->d_sel_count, h->max_frames); }

int ensure_detect_scratch(lf_mkd *h) {
    if (h->d_slots) return LF_MKD_OK;
    int gx, gy, gz;
    scan_grid(int(h->params.max_image_width), int(h->params.max_image_height), h->n_layers - 1, kBorder, kSkipLayers, gx,
              gy, gz);
    const size_t cubes = std::max<size_t>(size_t(gx) * gy * gz, 1) * h->max_frames;
    if (int rc = grow(h, h->d_slots, cubes * 8 * 4)) return rc;
    if (int rc = grow(h, h->d_cube_counts, cubes)) return rc;
    if (int rc = grow(h, h->d_cube_sums, (cubes + 1023) / 1024 + 1)) return rc;
    return ensure_sel_count(h);
}

// ordered extrema of all loaded frames into d_out (device), counts to the host
int detect_extrema_device(lf_mkd *h, float *d_out, uint32_t *d_frame_of, uint64_t max_out, uint64_t *n_out,
                          uint64_t *n_dropped, hipStream_t s) {
    if (int rc = ensure_coarse_stack(h, s)) return rc;
    if (int rc = ensure_detect_scratch(h)) return rc;
    launch_detect_extrema(h->d_pyr + h->pd.offset[0], h->pyr_stride, h->pd.pitch[0], h->d_coarse, h->coarse_stride, h->layer_stride,
                          h->n_layers, h->pd.w[0], h->pd.h[0], int(h->n_frames), kBorder, kSkipLayers, kContrastThreshold,
                          h->d_slots, h->d_cube_counts, h->d_cube_sums, d_out, d_frame_of, nullptr, max_out, h->d_totals,
                          s);
    LF_HIP(h, hipGetLastError());
    unsigned long long totals[2] = {0, 0};
    LF_HIP(h, hipMemcpyAsync(totals, h->d_totals, sizeof(totals), hipMemcpyDeviceToHost, s));
    LF_HIP(h, hipStreamSynchronize(s));
    *n_out = totals[0];
    if (n_dropped) *n_dropped = totals[1];
    return LF_MKD_OK;
}

// scratch of the long-list top-n selection; its histograms are zero between uses (the selection's last launch leaves them
// so), which a fresh allocation has to establish once
// (zeroed on the stream the selection will run on, outside any capture: the consumers' streams are non-blocking, i.e. not
// ordered with the null stream)
int grow_topk_work(lf_mkd *h, uint64_t n_cap, hipStream_t s) {
    const uint64_t before = h->d_topk_work.cap();
    if (int rc = grow(h, h->d_topk_work, topk_work_words(n_cap))) return rc;
    if (h->d_topk_work.cap() != before) LF_HIP(h, hipMemsetAsync(h->d_topk_work, 0, topk_work_words(n_cap) * 4, s));
    return LF_MKD_OK;
}

int orient_device(lf_mkd *h, const float *d_extrema, const uint32_t *d_frame_of, uint64_t n, float *d_out,
                  uint32_t *d_frame_of_kp, uint64_t max_out, uint64_t *n_out, uint64_t *n_dropped, hipStream_t s) {
    if (int rc = ensure_coarse_stack(h, s)) return rc;
    launch_orient(h->d_pyr + h->pd.offset[0], h->pyr_stride, h->pd.pitch[0], h->d_coarse, h->coarse_stride, h->layer_stride, h->n_layers,
                  h->pd.w[0], h->pd.h[0], d_extrema, d_frame_of, long(n), nullptr, h->d_angles, h->d_counts,
                  h->d_orient_sums, d_out, d_frame_of_kp, max_out, h->d_totals, s);
    LF_HIP(h, hipGetLastError());
    unsigned long long totals[2] = {0, 0};
    LF_HIP(h, hipMemcpyAsync(totals, h->d_totals, sizeof(totals), hipMemcpyDeviceToHost, s));
    LF_HIP(h, hipStreamSynchronize(s));
    *n_out = totals[0];
    if (n_dropped) *n_dropped = totals[1];
    return LF_MKD_OK;
}

// ---- the banded upload's plan (lf_mkd_detect / lf_mkd_detect_u8 on large frames) --------------------------------------
// Stage rows [lo, hi) of piece p of a frame cut at raw rows cuts[0] < cuts[1] < ... < h (the last piece ends at h).
bool piece_bands(const std::vector<uint32_t> &cuts, size_t p, int w, int hgt, int n_layers, RowBands &b) {
    RowBands lo{}, hi{};
    if (p > 0 && !plan_row_bands(int(cuts[p - 1]), w, hgt, n_layers, kBorder, lo)) return false;
    const bool last = p == cuts.size();
    if (!last && !plan_row_bands(int(cuts[p]), w, hgt, n_layers, kBorder, hi)) return false;
    b = RowBands{};
    b.last = last ? 1 : 0;
    b.level0_lo = lo.level0_hi;
    b.level0_hi = last ? hgt : hi.level0_hi;
    for (int l = 0; l < 8; ++l) {
        b.layer_lo[l] = lo.layer_hi[l];
        b.layer_hi[l] = last ? hgt : hi.layer_hi[l];
    }
    b.scan_lo = lo.scan_hi;
    b.scan_hi = last ? (hgt - 2 * kBorder + 7) / 8 : hi.scan_hi;
    return true;
}

// What the pieces cost, from this chip's timelines of the reference benchmark's frame (4096 x 3072; profiles/r06_bands.md):
// picoseconds per pixel of a stage's rows plus a floor per launch; the link's rate for a copy from pageable memory and what
// an extra piece costs the link: ~11 us per copy call (r05_upload_probe.txt) + ~15 us in which the host, blocked in the
// copy until then, records the event and launches the head.
struct FrontModel {
    double sep3 = 2.3, swt = 1.7, swt_deep = 2.3, floor_us = 5.0, link_gb_s = 56.0, gap_us = 26.0;
    double scan(int n_fine) const { return std::max(3.25 * n_fine - 6.85, 2.0); }
};
// Modelled time (us) at which the device is through with the front's share of pieces 0 .. n_pieces-1 of a frame cut at
// `cuts` (n_pieces = cuts.size() + 1: the whole front); *link_us: when the last of these pieces has arrived.
double front_finish_us(const std::vector<uint32_t> &cuts, size_t n_pieces, int w, int hgt, int bpp, int n_layers,
                       const FrontModel &m, double *link_us = nullptr) {
    const double row_us = double(w) * bpp / (m.link_gb_s * 1e3);
    double t_link = 0, t_dev = 0;
    uint32_t from = 0;
    for (size_t p = 0; p < n_pieces; ++p) {
        const uint32_t to = p < cuts.size() ? cuts[p] : uint32_t(hgt);
        t_link += (p ? m.gap_us : 0.0) + double(to - from) * row_us;
        from = to;
        RowBands b;
        if (!piece_bands(cuts, p, w, hgt, n_layers, b)) return 1e30;
        double head = 0;
        auto add = [&](int rows, double ps) {
            if (rows > 0) head += m.floor_us + double(rows) * w * ps * 1e-6;
        };
        add(b.level0_hi - b.level0_lo, m.sep3);
        for (int l = 0; l + 1 < n_layers; ++l) add(b.layer_hi[l] - b.layer_lo[l], (1 << l) > 32 ? m.swt_deep : m.swt);
        add((b.scan_hi - b.scan_lo) * 8, m.scan(n_layers - 1));
        t_dev = std::max(t_dev, t_link) + head;
    }
    if (link_us) *link_us = t_link;
    return t_dev;
}

// Where to cut a frame of `bpp` bytes per pixel.  Candidates: k equal pieces, and plans in which every piece after the first
// is sized so that its upload ends when the device is through with the pieces before it (the link and the device both stay
// busy) -- an 8-bit frame, whose front takes longer than its upload, comes out as a small first piece and growing ones after
// it; an f32 frame, four times the bytes, as a large first piece and shrinking ones, so that little is left to do when the
// last byte lands.  The candidate with the earliest modelled finish wins; no cuts (one piece) unless it is ahead by 4 %.
// LF_MKD_DETECT_BANDS=0: one piece.  LF_MKD_BAND_SPLIT=f1[,f2..]: cuts at these fractions of the height;
// LF_MKD_BAND_PIECES=k: k equal pieces -- both whatever the frame's size (tests, A/B runs).
std::vector<uint32_t> plan_cuts(int n_layers, uint32_t width, uint32_t height, bool u8) {
    const std::vector<uint32_t> none;
    const int w = int(width), hgt = int(height), bpp = u8 ? 1 : 4;
    RowBands probe;
    // (a frame with a pyramid of one level -- fewer than 3 rows or columns -- has nothing to band)
    if (pyramid_levels(width, height) < 2 || height < 64 || !plan_row_bands(int(height) / 2 / 4 * 4, w, hgt, n_layers, kBorder, probe)) return none;
    // cuts on multiples of four rows, at least 16 rows from either end, strictly increasing
    auto valid = [&](std::vector<uint32_t> &c) {
        for (auto &r : c) r = std::min<uint32_t>(std::max<uint32_t>(r, 16), height - 16) / 4 * 4;
        c.erase(std::unique(c.begin(), c.end()), c.end());
        for (size_t i = 0; i < c.size(); ++i)
            if (c[i] >= height || (i && c[i] <= c[i - 1])) return false;
        return !c.empty();
    };
    const char *env_b = getenv("LF_MKD_DETECT_BANDS"), *env_f = getenv("LF_MKD_BAND_SPLIT"), *env_k = getenv("LF_MKD_BAND_PIECES");
    auto equal_pieces = [&](int k) {
        std::vector<uint32_t> c;
        for (int i = 1; i < k; ++i) c.push_back(uint32_t(uint64_t(height) * i / k));
        return c;
    };
    if (env_f) {
        std::vector<uint32_t> c;
        for (const char *q = env_f; *q;) {
            char *end = nullptr;
            const double f = strtod(q, &end);
            if (end == q) break;
            c.push_back(uint32_t(double(height) * (f >= 0.0 ? std::min(f, 1.0) : 0.0)));     // (a NaN counts as 0)
            q = *end == ',' ? end + 1 : end;
        }
        std::sort(c.begin(), c.end());
        return valid(c) ? c : none;
    }
    if (env_k) {
        std::vector<uint32_t> c = equal_pieces(std::min(std::max(atoi(env_k), 1), 16));
        return valid(c) ? c : none;
    }
    if ((env_b && env_b[0] == '0') || uint64_t(width) * height * bpp < 6000000ull) return none;
    const FrontModel m;
    const double row_us = double(w) * bpp / (m.link_gb_s * 1e3);
    std::vector<uint32_t> best;
    double best_t = front_finish_us(none, 1, w, hgt, bpp, n_layers, m) * 0.96;
    auto consider = [&](std::vector<uint32_t> c) {
        if (!valid(c)) return;
        const double t = front_finish_us(c, c.size() + 1, w, hgt, bpp, n_layers, m);
        if (t < best_t) {
            best_t = t;
            best = c;
        }
    };
    for (int k = 2; k <= 6; ++k) consider(equal_pieces(k));
    for (int i = 1; i <= 14; ++i) {             // first piece = i / 16 of the frame, the others by the recurrence
        std::vector<uint32_t> c{uint32_t(uint64_t(height) * i / 16)};
        while (c.size() < 6 && valid(c)) {
            consider(c);
            // the next piece: as many rows as the link delivers while the device works off the pieces so far
            double t_link = 0;
            const double t_dev = front_finish_us(c, c.size(), w, hgt, bpp, n_layers, m, &t_link);
            const uint32_t rows = uint32_t(std::max((t_dev - t_link - m.gap_us) / row_us, double(height) / 16));
            if (c.back() + rows + height / 16 >= height) break;
            c.push_back(c.back() + rows);
        }
    }
    return best;
}

}  // namespace

int lf_mkd_internal_device(const lf_mkd *h) { return h->params.device; }
hipStream_t lf_mkd_internal_stream(lf_mkd *h) { return h->stream; }
int lf_mkd_internal_fail(lf_mkd *h, int code, const std::string &msg) { return fail(h, code, msg); }

extern "C" {

const char *lf_mkd_version(void) { return "lf_mkd 0.1.0 gfx950"; }

int lf_mkd_create(const lf_mkd_params *params, const float *mean, const float *eigvals, const float *eigvecs,
                  lf_mkd **out) {
    if (!mean || !eigvals || !eigvecs) return LF_MKD_ERR_BAD_ARG;
    PcaModel pca;
    pca.mean.assign(mean, mean + kRaw);
    pca.eigvals.assign(eigvals, eigvals + kRaw);
    pca.eigvecs.assign(eigvecs, eigvecs + size_t(kRaw) * kRaw);
    return create_impl(params, pca, out);
}

int lf_mkd_build_constants(const float *mean, const float *eigvals, const float *eigvecs, float *gradient_angle,
                           float *embedding_polar, float *embedding_cartesian, float *w_t) {
    if (!mean || !eigvals || !eigvecs) return LF_MKD_ERR_BAD_ARG;
    PcaModel pca;
    pca.mean.assign(mean, mean + kRaw);
    pca.eigvals.assign(eigvals, eigvals + kRaw);
    pca.eigvecs.assign(eigvecs, eigvecs + size_t(kRaw) * kRaw);
    HostConsts hc;
    if (const std::string e = build_host_consts(pca, hc); !e.empty()) {
        g_create_error = e;
        return LF_MKD_ERR_BAD_ARG;
    }
    if (gradient_angle) std::memcpy(gradient_angle, hc.gradient_angle.data(), hc.gradient_angle.size() * 4);
    if (embedding_polar) std::memcpy(embedding_polar, hc.embedding_polar.data(), hc.embedding_polar.size() * 4);
    if (embedding_cartesian)
        std::memcpy(embedding_cartesian, hc.embedding_cartesian.data(), hc.embedding_cartesian.size() * 4);
    if (w_t) std::memcpy(w_t, hc.w_t.data(), hc.w_t.size() * 4);
    return LF_MKD_OK;
}

// Test-only tap (not part of include/lf_mkd.h): the folded pooling tables as the handle would upload them.
//   pool_b_f32 [32][12][2][64][4], colmap [336], parity_defect [1]; any of them may be null
int lfmkd_test_pool_tables(const float *mean, const float *eigvals, const float *eigvecs, float *pool_b_f32, int16_t *colmap, float *parity_defect) {
    if (!mean || !eigvals || !eigvecs) return LF_MKD_ERR_BAD_ARG;
    PcaModel pca;
    pca.mean.assign(mean, mean + kRaw);
    pca.eigvals.assign(eigvals, eigvals + kRaw);
    pca.eigvecs.assign(eigvecs, eigvecs + size_t(kRaw) * kRaw);
    HostConsts hc;
    if (const std::string e = build_host_consts(pca, hc); !e.empty()) {
        g_create_error = e;
        return LF_MKD_ERR_BAD_ARG;
    }
    if (pool_b_f32) std::memcpy(pool_b_f32, hc.pool_b_f32.data(), hc.pool_b_f32.size() * 4);
    if (colmap) std::memcpy(colmap, hc.colmap.data(), hc.colmap.size() * 2);
    if (parity_defect) *parity_defect = hc.lut_parity_defect;
    return LF_MKD_OK;
}

// Test-only tap (not part of include/lf_mkd.h): the factors LF_MKD_POOL_F16X3 pools the x-odd cartesian kernels with.
//   fx [16], gy [32][4], defect [1] (HostConsts::odd_cart_*); any of them may be null
int lfmkd_test_pool_factors(const float *mean, const float *eigvals, const float *eigvecs, float *fx, float *gy, float *defect) {
    if (!mean || !eigvals || !eigvecs) return LF_MKD_ERR_BAD_ARG;
    PcaModel pca;
    pca.mean.assign(mean, mean + kRaw);
    pca.eigvals.assign(eigvals, eigvals + kRaw);
    pca.eigvecs.assign(eigvecs, eigvecs + size_t(kRaw) * kRaw);
    HostConsts hc;
    if (const std::string e = build_host_consts(pca, hc); !e.empty()) {
        g_create_error = e;
        return LF_MKD_ERR_BAD_ARG;
    }
    if (fx) std::memcpy(fx, hc.odd_cart_fx, sizeof hc.odd_cart_fx);
    if (gy) std::memcpy(gy, hc.odd_cart_gy, sizeof hc.odd_cart_gy);
    if (defect) *defect = hc.odd_cart_defect;
    return LF_MKD_OK;
}

int lf_mkd_plan_upload(uint32_t width, uint32_t height, uint32_t bytes_per_pixel, uint32_t n_scales, uint32_t *cuts,
                       uint32_t max_cuts, uint32_t *n_cuts, double *modelled_us, double *one_piece_us) {
    if (!n_cuts || (bytes_per_pixel != 1 && bytes_per_pixel != 4) || width < 2 || height < 2 || (max_cuts && !cuts))
        return LF_MKD_ERR_BAD_ARG;
    const int n_layers = int(n_scales ? n_scales : 4) + 3;
    if (n_layers - 1 > 8) return LF_MKD_ERR_BAD_ARG;
    const std::vector<uint32_t> c = plan_cuts(n_layers, width, height, bytes_per_pixel == 1);
    *n_cuts = uint32_t(c.size());
    for (size_t i = 0; i < c.size() && i < max_cuts; ++i) cuts[i] = c[i];
    const FrontModel m;
    if (modelled_us) *modelled_us = front_finish_us(c, c.size() + 1, int(width), int(height), int(bytes_per_pixel), n_layers, m);
    if (one_piece_us) *one_piece_us = front_finish_us({}, 1, int(width), int(height), int(bytes_per_pixel), n_layers, m);
    return LF_MKD_OK;
}

int lf_mkd_create_from_file(const lf_mkd_params *params, const char *path, lf_mkd **out) {
    if (!path) return LF_MKD_ERR_BAD_ARG;
    PcaModel pca;
    const std::string e = load_pca_safetensors(path, pca);
    if (!e.empty()) {
        g_create_error = e;
        return LF_MKD_ERR_IO;
    }
    return create_impl(params, pca, out);
}

void lf_mkd_destroy(lf_mkd *h) {
    if (!h) return;
    lfmkd::DeviceScope scope_;
    (void)scope_.enter(h->params.device);
    (void)hipDeviceSynchronize();   // work of this handle may be in flight on the caller's streams too
    h->stream_graph.reset();        // the recordings, then the events and streams; the arrays go with the handle
    h->plans.clear();
    for (const std::vector<hipEvent_t> *events : {&h->copy_ev, &h->ev_pending, &h->ev_free, &h->side_events})
        for (hipEvent_t e : *events) (void)hipEventDestroy(e);
    for (hipEvent_t e : h->det_ev)
        if (e) (void)hipEventDestroy(e);
    for (hipStream_t s : {h->copy_stream, h->side_stream, h->stream})
        if (s) (void)hipStreamDestroy(s);
    delete h;
}

const char *lf_mkd_last_error(const lf_mkd *h) { return h ? h->err.c_str() : g_create_error.c_str(); }

int lf_mkd_kernel_times(lf_mkd *h, double *pool_ms, double *whiten_ms, uint64_t *launches) {
    if (!h) return LF_MKD_ERR_BAD_ARG;
    LF_ENTER(h);
    double tp = 0, tw = 0;
    const size_t nb = h->ev_pending.size() / 2;
    for (size_t i = 0; i < nb; ++i) {
        float a = 0;
        LF_HIP(h, hipEventSynchronize(h->ev_pending[2 * i + 1]));
        LF_HIP(h, hipEventElapsedTime(&a, h->ev_pending[2 * i], h->ev_pending[2 * i + 1]));
        tp += a;
    }
    h->ev_free.insert(h->ev_free.end(), h->ev_pending.begin(), h->ev_pending.end());
    h->ev_pending.clear();
    if (pool_ms) *pool_ms = tp;
    if (whiten_ms) *whiten_ms = tw;
    if (launches) *launches = nb;
    return LF_MKD_OK;
}

int lf_mkd_kernel_clock(lf_mkd *h, void *stream, double *shader_mhz, double *kernel_ms) {
    if (!h) return LF_MKD_ERR_BAD_ARG;
    if (shader_mhz) *shader_mhz = 0;
    if (kernel_ms) *kernel_ms = 0;
    if (!h->d_clk) return fail(h, LF_MKD_ERR_BAD_ARG, "kernel_clock: the handle was not created with LF_MKD_FLAG_KERNEL_TIMING");
    LF_ENTER(h);
    hipStream_t s = stream_of(h, stream);
    unsigned long long c[4] = {0, 0, 0, 0};
    LF_HIP(h, hipMemcpyAsync(c, h->d_clk, sizeof(c), hipMemcpyDeviceToHost, s));
    LF_HIP(h, hipStreamSynchronize(s));
    if (c[3] > c[1] && c[2] > c[0]) {
        const double ticks = double(c[3] - c[1]);            // s_memrealtime: 100 MHz
        if (shader_mhz) *shader_mhz = double(c[2] - c[0]) / ticks * 100.0;
        if (kernel_ms) *kernel_ms = ticks / 1e5;
    }
    return LF_MKD_OK;
}

int lf_mkd_synchronize(lf_mkd *h) {
    if (!h) return LF_MKD_ERR_BAD_ARG;
    LF_ENTER(h);
    LF_HIP(h, hipStreamSynchronize(h->stream));
    return LF_MKD_OK;
}

int lf_mkd_describe_patches_device(lf_mkd *h, const float *d_patches, uint64_t n, float *d_out, void *stream) {
    if (!h) return LF_MKD_ERR_BAD_ARG;
    if (n == 0) return LF_MKD_OK;
    if (!d_patches || !d_out) return fail(h, LF_MKD_ERR_BAD_ARG, "describe_patches_device: null pointer");
    LF_ENTER(h);
    hipStream_t s = stream_of(h, stream);
    for (uint64_t off = 0; off < n; off += h->batch) {
        const uint64_t m = std::min<uint64_t>(h->batch, n - off);
        const int rc = run_batch(h, d_patches + off * kPx, m, d_out + off * kOut, nullptr, s);
        if (rc) return rc;
    }
    return LF_MKD_OK;
}

int lf_mkd_raw_descriptors_device(lf_mkd *h, const float *d_patches, uint64_t n, float *d_raw, void *stream) {
    if (!h) return LF_MKD_ERR_BAD_ARG;
    if (n == 0) return LF_MKD_OK;
    if (!d_patches || !d_raw) return fail(h, LF_MKD_ERR_BAD_ARG, "raw_descriptors_device: null pointer");
    LF_ENTER(h);
    if (int rc = ensure_staging(h)) return rc;   // the kernel also writes the whitened descriptors: into the staging buffer
    hipStream_t s = stream_of(h, stream);
    for (uint64_t off = 0; off < n; off += h->batch) {
        const uint64_t m = std::min<uint64_t>(h->batch, n - off);
        const int rc = run_batch(h, d_patches + off * kPx, m, nullptr, d_raw + off * kRaw, s);
        if (rc) return rc;
    }
    return LF_MKD_OK;
}

int lf_mkd_describe_patches(lf_mkd *h, const float *patches, uint64_t n, float *out) {
    if (!h) return LF_MKD_ERR_BAD_ARG;
    if (n == 0) return LF_MKD_OK;
    if (!patches || !out) return fail(h, LF_MKD_ERR_BAD_ARG, "describe_patches: null pointer");
    LF_ENTER(h);
    if (int rc = ensure_staging(h)) return rc;
    for (uint64_t off = 0; off < n; off += h->batch) {
        const uint64_t m = std::min<uint64_t>(h->batch, n - off);
        LF_HIP(h, hipMemcpyAsync(h->d_patches, patches + off * kPx, m * kPx * 4, hipMemcpyHostToDevice, h->stream));
        const int rc = run_batch(h, h->d_patches, m, h->d_out, nullptr, h->stream);
        if (rc) return rc;
        LF_HIP(h, hipMemcpyAsync(out + off * kOut, h->d_out, m * kOut * 4, hipMemcpyDeviceToHost, h->stream));
        LF_HIP(h, hipStreamSynchronize(h->stream));
    }
    return LF_MKD_OK;
}

// lf_mkd_set_images_device and its 8-bit twin: exactly one of d_images / d_images_u8 is given
static int set_images_impl(lf_mkd *h, const float *d_images, const unsigned char *d_images_u8, uint32_t n_frames,
                           uint32_t width, uint32_t height, void *stream) {
    if (!h) return LF_MKD_ERR_BAD_ARG;
    if ((!d_images && !d_images_u8) || width < 2 || height < 2 || n_frames == 0)
        return fail(h, LF_MKD_ERR_BAD_ARG, "set_image: bad image");
    if (!h->d_pyr || width > h->params.max_image_width || height > h->params.max_image_height)
        return fail(h, LF_MKD_ERR_BAD_ARG,
                    "set_image: image " + std::to_string(width) + "x" + std::to_string(height) +
                        " exceeds max_image_width/height given at creation");
    if (n_frames > h->max_frames)
        return fail(h, LF_MKD_ERR_BAD_ARG, "set_images: " + std::to_string(n_frames) + " frames exceed max_frames = " +
                                               std::to_string(h->max_frames) + " given at creation");
    LF_ENTER(h);
    hipStream_t s = stream_of(h, stream);
    describe_pyramid(width, height, h->pd);
    // once the a-trous stack exists (orientation or the detector have been used on this handle) the pyramid's
    // a-trous layer 1 goes straight into it
    const bool share = h->d_coarse.get() != nullptr && h->pd.levels >= 2;
    launch_build_pyramid(d_images, long(width) * height, h->d_pyr, h->pyr_stride, h->d_tmp_a, h->d_tmp_b, h->pd,
                         int(n_frames), share ? h->d_coarse.get() : nullptr, h->coarse_stride, s, nullptr, nullptr, nullptr, {},
                         d_images_u8);
    h->coarse_l1_valid = share;
    LF_HIP(h, hipGetLastError());
    h->have_image = true;
    h->coarse_valid = false;
    h->n_frames = n_frames;
    return LF_MKD_OK;
}

int lf_mkd_set_images_device(lf_mkd *h, const float *d_images, uint32_t n_frames, uint32_t width, uint32_t height,
                             void *stream) {
    if (h && !d_images) return fail(h, LF_MKD_ERR_BAD_ARG, "set_image: bad image");
    return set_images_impl(h, d_images, nullptr, n_frames, width, height, stream);
}

int lf_mkd_set_images_u8_device(lf_mkd *h, const uint8_t *d_images, uint32_t n_frames, uint32_t width, uint32_t height,
                                void *stream) {
    if (h && !d_images) return fail(h, LF_MKD_ERR_BAD_ARG, "set_image_u8: bad image");
    return set_images_impl(h, nullptr, d_images, n_frames, width, height, stream);
}

int lf_mkd_set_image_device(lf_mkd *h, const float *d_image, uint32_t width, uint32_t height, void *stream) {
    return lf_mkd_set_images_device(h, d_image, 1, width, height, stream);
}

// the 8-bit staging frame (1 B/px; lf_mkd_set_image_u8, lf_mkd_detect_u8), allocated on first use
// (a recorded pipeline reads it by address: allocated once at the maximum frame size, it never moves)
static int ensure_u8_staging(lf_mkd *h) {
    return grow(h, h->d_image_u8, (size_t(h->params.max_image_width) * h->params.max_image_height + 3) / 4 * 4);
}

int lf_mkd_set_image(lf_mkd *h, const float *image, uint32_t width, uint32_t height) {
    if (!h) return LF_MKD_ERR_BAD_ARG;
    if (!image) return fail(h, LF_MKD_ERR_BAD_ARG, "set_image: null image");
    if (!h->d_image || width > h->params.max_image_width || height > h->params.max_image_height)
        return fail(h, LF_MKD_ERR_BAD_ARG, "set_image: image exceeds max_image_width/height given at creation");
    LF_ENTER(h);
    LF_HIP(h, hipMemcpyAsync(h->d_image, image, size_t(width) * height * 4, hipMemcpyHostToDevice, h->stream));
    const int rc = lf_mkd_set_image_device(h, h->d_image, width, height, h->stream);
    if (rc) return rc;
    LF_HIP(h, hipStreamSynchronize(h->stream));
    return LF_MKD_OK;
}

int lf_mkd_set_image_u8(lf_mkd *h, const uint8_t *image, uint32_t width, uint32_t height) {
    if (!h) return LF_MKD_ERR_BAD_ARG;
    if (!image) return fail(h, LF_MKD_ERR_BAD_ARG, "set_image_u8: null image");
    if (!h->d_image || width > h->params.max_image_width || height > h->params.max_image_height)
        return fail(h, LF_MKD_ERR_BAD_ARG, "set_image_u8: image exceeds max_image_width/height given at creation");
    LF_ENTER(h);
    if (int rc = ensure_u8_staging(h)) return rc;
    LF_HIP(h, hipMemcpyAsync(h->d_image_u8, image, size_t(width) * height, hipMemcpyHostToDevice, h->stream));
    const int rc = lf_mkd_set_images_u8_device(h, h->d_image_u8, 1, width, height, h->stream);
    if (rc) return rc;
    LF_HIP(h, hipStreamSynchronize(h->stream));
    return LF_MKD_OK;
}

int lf_mkd_sample_patches_device(lf_mkd *h, const lf_mkd_keypoint *d_kps, uint64_t n, float *d_patches,
                                 void *stream) {
    if (!h) return LF_MKD_ERR_BAD_ARG;
    if (!h->have_image) return fail(h, LF_MKD_ERR_NO_IMAGE, "sample_patches: call lf_mkd_set_image first");
    if (n == 0) return LF_MKD_OK;
    if (!d_kps || !d_patches) return fail(h, LF_MKD_ERR_BAD_ARG, "sample_patches: null pointer");
    LF_ENTER(h);
    hipStream_t s = stream_of(h, stream);
    launch_sample_patches(h->d_pyr, h->pyr_stride, h->pd, reinterpret_cast<const float *>(d_kps), nullptr, 1, long(n),
                          nullptr, h->params.patch_scale_factor, d_patches, s);
    LF_HIP(h, hipGetLastError());
    return LF_MKD_OK;
}

int lf_mkd_describe_keypoints_frames_device(lf_mkd *h, const lf_mkd_keypoint *d_kps, const uint32_t *d_frame_of_kp,
                                            uint64_t n, float *d_out, void *stream) {
    if (!h) return LF_MKD_ERR_BAD_ARG;
    if (!h->have_image) return fail(h, LF_MKD_ERR_NO_IMAGE, "describe_keypoints: call lf_mkd_set_image first");
    if (n == 0) return LF_MKD_OK;
    if (!d_kps || !d_out) return fail(h, LF_MKD_ERR_BAD_ARG, "describe_keypoints_device: null pointer");
    LF_ENTER(h);
    hipStream_t s = stream_of(h, stream);
    return describe_keypoints_on_device(h, reinterpret_cast<const float *>(d_kps), d_frame_of_kp, n, d_out, s);
}

int lf_mkd_describe_keypoints_device(lf_mkd *h, const lf_mkd_keypoint *d_kps, uint64_t n, float *d_out,
                                     void *stream) {
    return lf_mkd_describe_keypoints_frames_device(h, d_kps, nullptr, n, d_out, stream);
}

int lf_mkd_describe_keypoints(lf_mkd *h, const lf_mkd_keypoint *kps, uint64_t n, float *out) {
    if (!h) return LF_MKD_ERR_BAD_ARG;
    if (!h->have_image) return fail(h, LF_MKD_ERR_NO_IMAGE, "describe_keypoints: call lf_mkd_set_image first");
    if (n == 0) return LF_MKD_OK;
    if (!kps || !out) return fail(h, LF_MKD_ERR_BAD_ARG, "describe_keypoints: null pointer");
    LF_ENTER(h);
    if (int rc = ensure_io_staging(h)) return rc;
    for (uint64_t off = 0; off < n; off += h->batch) {
        const uint64_t m = std::min<uint64_t>(h->batch, n - off);
        LF_HIP(h, hipMemcpyAsync(h->d_kps, kps + off, m * sizeof(lf_mkd_keypoint), hipMemcpyHostToDevice, h->stream));
        if (int rc = describe_keypoints_on_device(h, h->d_kps, nullptr, m, h->d_out, h->stream)) return rc;
        LF_HIP(h, hipMemcpyAsync(out + off * kOut, h->d_out, m * kOut * 4, hipMemcpyDeviceToHost, h->stream));
        LF_HIP(h, hipStreamSynchronize(h->stream));
    }
    if (h->d_kp_words) {   // the row-split form counts partial sums that never reached their consumer (none, ever: a fault if so)
        unsigned lost = 0;
        LF_HIP(h, hipMemcpy(&lost, h->d_kp_words, 4, hipMemcpyDeviceToHost));
        if (lost) {
            (void)hipMemset(h->d_kp_words, 0, kp_split_counter_words(h->num_cus) * 4);
            return fail(h, LF_MKD_ERR_HIP, "describe_keypoints: " + std::to_string(lost) + " partial sums of the row-split form did not arrive");
        }
    }
    return LF_MKD_OK;
}

int lf_mkd_orient_keypoints_device(lf_mkd *h, const lf_mkd_extremum *d_extrema, const uint32_t *d_frame_of_extremum,
                                   uint64_t n, lf_mkd_keypoint *d_out, uint32_t *d_frame_of_kp, uint64_t max_out,
                                   uint64_t *n_out, uint64_t *n_dropped, void *stream) {
    if (!h) return LF_MKD_ERR_BAD_ARG;
    if (!n_out) return fail(h, LF_MKD_ERR_BAD_ARG, "orient_keypoints_device: n_out is null");
    *n_out = 0;
    if (n_dropped) *n_dropped = 0;
    if (!h->have_image) return fail(h, LF_MKD_ERR_NO_IMAGE, "orient_keypoints: call lf_mkd_set_image first");
    if (n == 0) return LF_MKD_OK;
    if (!d_extrema || (!d_out && max_out)) return fail(h, LF_MKD_ERR_BAD_ARG, "orient_keypoints_device: null pointer");
    LF_ENTER(h);
    hipStream_t s = stream_of(h, stream);
    if (int rc = ensure_orient_scratch(h, n, false, 0)) return rc;
    return orient_device(h, reinterpret_cast<const float *>(d_extrema), d_frame_of_extremum, n,
                         reinterpret_cast<float *>(d_out), d_frame_of_kp, max_out, n_out, n_dropped, s);
}

int lf_mkd_orient_keypoints(lf_mkd *h, const lf_mkd_extremum *extrema, uint64_t n, lf_mkd_keypoint *out,
                            uint64_t max_out, uint64_t *n_out, uint64_t *n_dropped) {
    if (!h) return LF_MKD_ERR_BAD_ARG;
    if (!n_out) return fail(h, LF_MKD_ERR_BAD_ARG, "orient_keypoints: n_out is null");
    *n_out = 0;
    if (n_dropped) *n_dropped = 0;
    if (!h->have_image) return fail(h, LF_MKD_ERR_NO_IMAGE, "orient_keypoints: call lf_mkd_set_image first");
    if (n == 0) return LF_MKD_OK;
    if (!extrema || (!out && max_out)) return fail(h, LF_MKD_ERR_BAD_ARG, "orient_keypoints: null pointer");
    LF_ENTER(h);
    if (int rc = ensure_orient_scratch(h, n, true, std::max<uint64_t>(max_out, 1))) return rc;
    LF_HIP(h, hipMemcpyAsync(h->d_extrema, extrema, n * sizeof(lf_mkd_extremum), hipMemcpyHostToDevice, h->stream));
    if (int rc = orient_device(h, h->d_extrema.as<float>(), nullptr, n, h->d_kps_out.as<float>(), nullptr, max_out, n_out,
                               n_dropped, h->stream))
        return rc;
    if (*n_out) LF_HIP(h, hipMemcpy(out, h->d_kps_out, *n_out * sizeof(lf_mkd_keypoint), hipMemcpyDeviceToHost));
    return LF_MKD_OK;
}

int lf_mkd_detect_extrema_device(lf_mkd *h, lf_mkd_extremum *d_out, uint32_t *d_frame_of, uint64_t max_out,
                                 uint64_t *n_out, uint64_t *n_dropped, void *stream) {
    if (!h) return LF_MKD_ERR_BAD_ARG;
    if (!n_out) return fail(h, LF_MKD_ERR_BAD_ARG, "detect_extrema_device: n_out is null");
    *n_out = 0;
    if (n_dropped) *n_dropped = 0;
    if (!h->have_image) return fail(h, LF_MKD_ERR_NO_IMAGE, "detect_extrema: call lf_mkd_set_image first");
    if (!d_out && max_out) return fail(h, LF_MKD_ERR_BAD_ARG, "detect_extrema_device: null pointer");
    LF_ENTER(h);
    hipStream_t s = stream_of(h, stream);
    return detect_extrema_device(h, reinterpret_cast<float *>(d_out), d_frame_of, max_out, n_out, n_dropped, s);
}

int lf_mkd_detect_extrema(lf_mkd *h, lf_mkd_extremum *out, uint64_t max_out, uint64_t *n_out, uint64_t *n_dropped) {
    if (!h) return LF_MKD_ERR_BAD_ARG;
    if (!n_out) return fail(h, LF_MKD_ERR_BAD_ARG, "detect_extrema: n_out is null");
    *n_out = 0;
    if (n_dropped) *n_dropped = 0;
    if (!h->have_image) return fail(h, LF_MKD_ERR_NO_IMAGE, "detect_extrema: call lf_mkd_set_image first");
    if (!out && max_out) return fail(h, LF_MKD_ERR_BAD_ARG, "detect_extrema: null pointer");
    LF_ENTER(h);
    if (int rc = grow(h, h->d_det_extrema, max_out)) return rc;
    if (int rc = detect_extrema_device(h, h->d_det_extrema.as<float>(), nullptr, max_out, n_out, n_dropped, h->stream)) return rc;
    if (*n_out) LF_HIP(h, hipMemcpy(out, h->d_det_extrema, *n_out * sizeof(lf_mkd_extremum), hipMemcpyDeviceToHost));
    return LF_MKD_OK;
}

int lf_mkd_filter_extrema_device(lf_mkd *h, const lf_mkd_extremum *d_extrema, uint64_t n, uint32_t top_n, float min_size,
                                 lf_mkd_extremum *d_out, uint32_t *d_index, uint64_t *n_out, void *stream) {
    if (!h) return LF_MKD_ERR_BAD_ARG;
    if (!n_out) return fail(h, LF_MKD_ERR_BAD_ARG, "filter_extrema_device: n_out is null");
    *n_out = 0;
    if (n == 0 || top_n == 0) return LF_MKD_OK;
    if (!d_extrema || !d_out) return fail(h, LF_MKD_ERR_BAD_ARG, "filter_extrema_device: null pointer");
    if (n > 0xFFFFFFFFull) return fail(h, LF_MKD_ERR_BAD_ARG, "filter_extrema_device: more than 2^32 extrema");
    LF_ENTER(h);
    hipStream_t s = stream_of(h, stream);
    if (int rc = ensure_sel_count(h)) return rc;
    if (int rc = grow_topk_work(h, n, s)) return rc;
    launch_topk_filter(reinterpret_cast<const float *>(d_extrema), nullptr, nullptr, n, 1, 0xFFFFFFFFu, top_n, min_size,
                       reinterpret_cast<float *>(d_out), d_index, h->d_sel_count, nullptr, n, h->d_topk_work, s);
    LF_HIP(h, hipGetLastError());
    unsigned cnt = 0;
    LF_HIP(h, hipMemcpyAsync(&cnt, h->d_sel_count, 4, hipMemcpyDeviceToHost, s));
    LF_HIP(h, hipStreamSynchronize(s));
    *n_out = cnt;
    return LF_MKD_OK;
}

// lf_mkd_detect stage by stage, every count fetched by the host before the next stage is sized (three waits on the stream):
// how the call worked before round 5, kept as the verification form (LF_MKD_FLAG_DETECT_STEPWISE) and for max_out == 0.
// The frame is already on the device (d_image or d_image_u8).
static int detect_stepwise(lf_mkd *h, bool u8, uint32_t width, uint32_t height, uint32_t top_n, float min_size,
                           lf_mkd_keypoint *keypoints, float *descriptors, uint64_t max_out, uint64_t *n_out,
                           uint64_t *dropped_blobs, uint64_t *dropped_features) {
    hipStream_t s = h->stream;
    // lf_mkd_set_image without its synchronisation, and -- once the a-trous stack exists, i.e. from the second call on --
    // with pyramid levels >= 1 (read by the sampler only) built on the side stream beside the a-trous passes and the scan
    describe_pyramid(width, height, h->pd);
    const bool share = h->d_coarse.get() != nullptr && h->pd.levels >= 2;
    if (share)
        if (int rc = ensure_side_stream(h, 2)) return rc;
    // (with the branch, the rest of the a-trous stack is queued from inside, ahead of it: see launch_build_pyramid)
    bool stack_queued = false;
    std::function<void()> stack_first;
    if (share)
        stack_first = [&] {
            launch_build_coarse_stack(h->d_pyr + h->pd.offset[0], h->pyr_stride, h->pd.pitch[0], h->d_coarse, h->coarse_stride,
                                      h->layer_stride, h->d_tmp_a, h->n_layers, 1, int(width), int(height), 1, s);
            stack_queued = true;
        };
    launch_build_pyramid(h->d_image, long(width) * height, h->d_pyr, h->pyr_stride, h->d_tmp_a, h->d_tmp_b, h->pd, 1,
                         share ? h->d_coarse.get() : nullptr, h->coarse_stride, s, share ? h->side_stream : nullptr,
                         share ? h->side_events[0] : nullptr, share ? h->side_events[1] : nullptr, stack_first,
                         u8 ? h->d_image_u8.get() : nullptr);
    LF_HIP(h, hipGetLastError());
    h->coarse_l1_valid = share;
    h->have_image = true;
    h->coarse_valid = stack_queued;
    h->n_frames = 1;
    // detect graph: extrema, at most max_extrema of them (mod.rs:625-633)
    if (int rc = grow(h, h->d_det_extrema, h->max_extrema)) return rc;
    uint64_t n_ext = 0;
    const int rc_ext = detect_extrema_device(h, h->d_det_extrema.as<float>(), nullptr, h->max_extrema, &n_ext, dropped_blobs, s);
    if (share) LF_HIP(h, hipStreamWaitEvent(s, h->side_events[1], 0));   // whatever follows on s sees the whole pyramid
    if (rc_ext) return rc_ext;
    // host blob filter of detect_top_n, on the device
    const float *d_sel = h->d_det_extrema.as<float>();
    if (top_n && n_ext) {
        if (int rc = grow(h, h->d_det_selected, top_n)) return rc;
        uint64_t n_sel = 0;
        if (int rc = lf_mkd_filter_extrema_device(h, h->d_det_extrema, n_ext, top_n, min_size, h->d_det_selected, nullptr,
                                                  &n_sel, s))
            return rc;
        d_sel = h->d_det_selected.as<float>();
        n_ext = n_sel;
    }
    if (n_ext == 0 || max_out == 0) return LF_MKD_OK;
    // extract graph: orientation, sampling, description
    if (int rc = ensure_orient_scratch(h, n_ext, true, max_out)) return rc;
    uint64_t n_kp = 0;
    if (int rc = orient_device(h, d_sel, nullptr, n_ext, h->d_kps_out.as<float>(), nullptr, max_out, &n_kp, dropped_features, s))
        return rc;
    if (n_kp == 0) return LF_MKD_OK;
    static_assert(sizeof(lf_mkd_keypoint) == 20, "keypoint layout");
    // (in the form the recorded pipeline takes for this request's max_out: the same bits)
    if (int rc = describe_keypoints_on_device(h, h->d_kps_out.as<float>(), nullptr, n_kp, h->d_det_desc, s, max_out)) return rc;
    LF_HIP(h, hipMemcpyAsync(keypoints, h->d_kps_out, n_kp * sizeof(lf_mkd_keypoint), hipMemcpyDeviceToHost, s));
    LF_HIP(h, hipMemcpyAsync(descriptors, h->d_det_desc, n_kp * kOut * 4, hipMemcpyDeviceToHost, s));
    LF_HIP(h, hipStreamSynchronize(s));
    *n_out = n_kp;
    return LF_MKD_OK;
}


// Everything a recorded pipeline for frames of width x height touches, allocated BEFORE the capture starts (an allocation
// inside a capture is an error, and one that moves a buffer retires every recording: retire_graph).
static int prepare_pipeline(lf_mkd *h, uint32_t top_n, uint64_t cap) {
    if (int rc = ensure_coarse_store(h)) return rc;
    if (int rc = ensure_detect_scratch(h)) return rc;
    if (int rc = grow(h, h->d_det_extrema, h->max_extrema)) return rc;
    if (top_n) {
        if (int rc = grow(h, h->d_det_selected, top_n)) return rc;
        if (int rc = grow_topk_work(h, h->max_extrema, h->stream)) return rc;
    }
    return ensure_orient_scratch(h, cap, false, 0);
}

// The launch sequence of lf_mkd_detect for frames of width x height read from d_image (f32) or d_image_u8 -- pyramid,
// a-trous stack, extremum scan, [top_n filter if top_n > 0], orientation, sampling + description -- with every count handed
// from stage to stage in device memory (cnt [8]: see lf_mkd_stream_create in lf_mkd.h).  host_counts (nullable, pinned): a
// last operation copies cnt there.  h->pd must describe the frame; every buffer must exist (prepare_pipeline), and the side
// stream when the frame has levels to build beside the detector.  Enqueued on the handle's stream: inside a capture
// (record_pipeline) or as it is (the first sighting of a request: the same launches, no recording, one wait).
static void enqueue_pipeline(lf_mkd *h, uint32_t width, uint32_t height, uint32_t top_n, float min_size, uint64_t max_out,
                             const float *d_image, const unsigned char *d_image_u8, lf_mkd_keypoint *d_keypoints,
                             float *d_descriptors, unsigned long long *cnt, unsigned long long *host_counts,
                             lf_mkd_keypoint *host_keypoints, const RowBands *bands) {
    hipStream_t s = h->stream;
    const uint64_t cap = top_n ? top_n : h->max_extrema;   // extrema that can reach orientation
    // the detector needs pyramid level 0 and a-trous layer 1 only: the other levels (read by the sampler at the very end)
    // are a branch beside the a-trous stack, the scan, the selection and the orientation
    const bool head_only = bands && !bands->last;           // (a piece's share: the front's kernels on its rows, nothing else)
    const bool fork = h->pd.levels >= 2 && !head_only;
    // (the a-trous stack is queued from inside, ahead of the branch: see launch_build_pyramid)
    launch_build_pyramid(d_image, long(width) * height, h->d_pyr, h->pyr_stride, h->d_tmp_a, h->d_tmp_b, h->pd, 1,
                         h->pd.levels >= 2 ? h->d_coarse.get() : nullptr, h->coarse_stride, s, fork ? h->side_stream : nullptr,
                         fork ? h->side_events[0] : nullptr, fork ? h->side_events[1] : nullptr, [&] {
                             launch_build_coarse_stack(h->d_pyr + h->pd.offset[0], h->pyr_stride, h->pd.pitch[0], h->d_coarse,
                                                       h->coarse_stride, h->layer_stride, h->d_tmp_a, h->n_layers,
                                                       h->pd.levels >= 2 ? 1 : 0, int(width), int(height), 1, s, bands);
                         }, d_image_u8, bands);
    launch_detect_extrema(h->d_pyr + h->pd.offset[0], h->pyr_stride, h->pd.pitch[0], h->d_coarse, h->coarse_stride, h->layer_stride,
                          h->n_layers, int(width), int(height), 1, kBorder, kSkipLayers, kContrastThreshold, h->d_slots,
                          h->d_cube_counts, h->d_cube_sums, h->d_det_extrema.as<float>(), nullptr, nullptr, h->max_extrema,
                          cnt + 0, s, bands);
    if (head_only) return;
    const float *d_sel = h->d_det_extrema.as<float>();
    const unsigned long long *n_sel = cnt + 0;
    if (top_n) {
        launch_topk_filter(d_sel, nullptr, cnt + 0, 0, 1, 0xFFFFFFFFu, top_n, min_size, h->d_det_selected.as<float>(), nullptr,
                           h->d_sel_count, cnt + 2, h->max_extrema, h->d_topk_work, s);
        d_sel = h->d_det_selected.as<float>();
        n_sel = cnt + 2;
    }
    launch_orient(h->d_pyr + h->pd.offset[0], h->pyr_stride, h->pd.pitch[0], h->d_coarse, h->coarse_stride, h->layer_stride, h->n_layers,
                  int(width), int(height), d_sel, nullptr, long(cap), n_sel, h->d_angles, h->d_counts, h->d_orient_sums,
                  reinterpret_cast<float *>(d_keypoints), nullptr, max_out, cnt + 3, s);
    // (the join costs ~12 us of queue latency wherever it stands, measured; the branch saves ~40)
    if (fork) (void)hipStreamWaitEvent(s, h->side_events[1], 0);
    if (fused_keypoints(h)) {
        launch_describe_keypoints(h->d_pyr, h->pyr_stride, h->pd, reinterpret_cast<const float *>(d_keypoints), nullptr, 1,
                                  long(max_out), cnt + 3, h->params.patch_scale_factor, h->dc, h->params.angle_mode,
                                  d_descriptors, h->num_cus, s, nullptr, h->d_kp_xchg, h->d_kp_words);
    } else {
        launch_sample_patches(h->d_pyr, h->pyr_stride, h->pd, reinterpret_cast<const float *>(d_keypoints), nullptr, 1,
                              long(max_out), cnt + 3, h->params.patch_scale_factor, h->d_stream_patches, s);
        launch_describe(h->d_stream_patches, long(max_out), cnt + 3, h->dc, h->params.angle_mode, h->params.pool_mode,
                        d_descriptors, nullptr, h->num_cus, s, 0, nullptr, h->next_claim());
    }
    // the counts and the keypoints go to pinned host memory as the last operations (on a branch of their own beside the describe
    // launch they were measured 15 us slower: every join of two branches costs ~12 us of queue latency)
    if (host_counts) (void)hipMemcpyAsync(host_counts, cnt, 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost, s);
    if (host_keypoints)
        (void)hipMemcpyAsync(host_keypoints, d_keypoints, max_out * sizeof(lf_mkd_keypoint), hipMemcpyDeviceToHost, s);
}

// Records that sequence as a hipGraph (the whole pipeline, or one piece's share of its front: bands).
static int record_pipeline(lf_mkd *h, uint32_t width, uint32_t height, uint32_t top_n, float min_size, uint64_t max_out,
                           const float *d_image, const unsigned char *d_image_u8, lf_mkd_keypoint *d_keypoints,
                           float *d_descriptors, unsigned long long *cnt, unsigned long long *host_counts,
                           lf_mkd_keypoint *host_keypoints, Recording &out, const RowBands *bands = nullptr) {
    hipStream_t s = h->stream;
    if (h->pd.levels >= 2 && !(bands && !bands->last))
        if (int rc = ensure_side_stream(h, 2)) return rc;
    LF_HIP(h, hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
    enqueue_pipeline(h, width, height, top_n, min_size, max_out, d_image, d_image_u8, d_keypoints, d_descriptors, cnt, host_counts,
                     host_keypoints, bands);
    Recording r;
    hipError_t e_end = hipStreamEndCapture(s, &r.graph);
    if (e_end != hipSuccess || !r.graph) {
        h->err = std::string("hipStreamEndCapture: ") + hipGetErrorString(e_end);
        return LF_MKD_ERR_HIP;
    }
    hipGraphExec_t exec = nullptr;
    hipError_t e_inst = hipGraphInstantiate(&exec, r.graph, nullptr, nullptr, 0);
    if (e_inst != hipSuccess) {
        h->err = std::string("hipGraphInstantiate: ") + hipGetErrorString(e_inst);
        return LF_MKD_ERR_HIP;
    }
    r.exec = exec;
    out = std::move(r);
    return LF_MKD_OK;
}

// LocalFeaturesVulkan::detect / detect_top_n (mod.rs:346-593) from a HOST frame, f32 or 8-bit.  A request (DetectKey) seen
// for the first time is served by the pipeline's own launches, not recorded (one upload, ~20 launches, one wait: no capture
// and no instantiation, which cost several times the call); the second time the pipeline is recorded (lf_mkd::sightings),
// and from then on a call is one upload (in planned pieces when the frame is large: plan_cuts), one launch of the recording,
// one wait, the result copies.  The reference's callers make this call per image (examples/match_images/src/main.rs:44-76:
// once per image, at its own size -- never a recording) or per camera frame (examples/webcam/src/main.rs:136-160).
enum class DetectForm { stepwise, direct, recorded };

static DetectForm choose_form(lf_mkd *h, const DetectKey &key) {
    // Stage by stage: when asked for (the verification flag), when only the counts are wanted, and on handles whose keypoint
    // mode takes the two-launch form (POOL_F32, F16_FP6, FLAG_UNFUSED_KEYPOINTS: verification forms whose staging patches
    // are sized by the internal batch there, by max_out x 4 KiB in a recording) ...
    if ((h->params.flags & LF_MKD_FLAG_DETECT_STEPWISE) || key.max_out == 0 || !fused_keypoints(h)) return DetectForm::stepwise;
    if (h->plans.find(key) || !h->record_after) return DetectForm::recorded;
    // ... or, while a request has not been seen record_after times, as the recording's own launches without recording them
    // (`direct`: every count handed on in device memory, one wait -- no capture, no instantiation, and none of the three
    // waits either)
    uint64_t *seen = h->sightings.find(key);
    if (!seen) {
        (void)h->sightings.make_room([] { return LF_MKD_OK; });
        seen = &h->sightings.add(key, 0);
    }
    if (*seen >= h->record_after) return DetectForm::recorded;
    ++*seen;
    return DetectForm::direct;
}

// The recording of `key`: large frames go over PCIe in pieces, and the pipeline's front runs on the rows a piece completes
// while the next one is on its way (RowBands; plan_cuts chooses the pieces).  h->pd must describe the frame.
static int record_plan(lf_mkd *h, const DetectKey &key, float min_size, DetectPlan &p) {
    p.cuts = h->pd.levels >= 2 ? plan_cuts(h->n_layers, key.w, key.h, key.u8) : std::vector<uint32_t>();
    if (!p.cuts.empty()) {
        if (!h->copy_stream) LF_HIP(h, hipStreamCreateWithFlags(&h->copy_stream, hipStreamNonBlocking));
        while (h->copy_ev.size() < p.cuts.size() + 1) {
            hipEvent_t e;
            LF_HIP(h, hipEventCreateWithFlags(&e, hipEventDisableTiming));
            h->copy_ev.push_back(e);
        }
    }
    RowBands bands{};
    for (size_t piece = 0; piece <= p.cuts.size(); ++piece) {
        if (!p.cuts.empty() && !piece_bands(p.cuts, piece, int(key.w), int(key.h), h->n_layers, bands))
            return fail(h, LF_MKD_ERR_BAD_ARG, "detect: internal error planning the banded upload");
        Recording r;
        if (int rc = record_pipeline(h, key.w, key.h, key.top_n, min_size, key.max_out, key.u8 ? nullptr : h->d_image.get(),
                                     key.u8 ? h->d_image_u8.get() : nullptr, h->d_kps_out, h->d_det_desc, h->d_det_counts,
                                     h->h_det_counts, h->h_res_kps, r, p.cuts.empty() ? nullptr : &bands))
            return rc;
        if (piece == p.cuts.size()) p.graph = std::move(r);
        else p.heads.push_back(std::move(r));
    }
    return LF_MKD_OK;
}

// The frame into d_image / d_image_u8: in one piece, or piece by piece by the plan's cuts (the call has waited for the device
// at its previous return: nothing still reads the staging frame) -- copy, then the head on the rows it completes, the next
// piece beside it.  A copy from pageable memory returns when its bytes are on their way, so the host is in the next copy
// while the device runs a head.
static int upload_frame(lf_mkd *h, const void *image, bool u8, uint32_t width, uint32_t height, const DetectPlan *plan) {
    hipStream_t s = h->stream;
    const size_t row = size_t(width) * (u8 ? 1 : 4);
    const unsigned char *src = static_cast<const unsigned char *>(image);
    unsigned char *dst = u8 ? h->d_image_u8.get() : h->d_image.as<unsigned char>();
    if (!plan || plan->cuts.empty()) {
        LF_HIP(h, hipMemcpyAsync(dst, src, row * height, hipMemcpyHostToDevice, s));
        return LF_MKD_OK;
    }
    size_t from = 0;
    for (size_t piece = 0; piece <= plan->cuts.size(); ++piece) {
        const size_t to = piece < plan->cuts.size() ? plan->cuts[piece] : height;
        LF_HIP(h, hipMemcpyAsync(dst + row * from, src + row * from, row * (to - from), hipMemcpyHostToDevice, h->copy_stream));
        LF_HIP(h, hipEventRecord(h->copy_ev[piece], h->copy_stream));
        LF_HIP(h, hipStreamWaitEvent(s, h->copy_ev[piece], 0));
        if (piece < plan->cuts.size()) LF_HIP(h, hipGraphLaunch(plan->heads[piece].exec, s));
        from = to;
    }
    return LF_MKD_OK;
}

// The results of a direct or recorded call, once the stream is through: the counts and the keypoints from the pinned copies
// the pipeline's last operations made, the descriptors by one copy of the n rows.
static int read_back(lf_mkd *h, bool timed, lf_mkd_keypoint *keypoints, float *descriptors, uint64_t max_out, uint64_t *n_out,
                     uint64_t *dropped_blobs, uint64_t *dropped_features) {
    hipStream_t s = h->stream;
    const auto t_back = std::chrono::steady_clock::now();
    if (timed) {
        float a = 0, b = 0;
        LF_HIP(h, hipEventElapsedTime(&a, h->det_ev[0], h->det_ev[1]));
        LF_HIP(h, hipEventElapsedTime(&b, h->det_ev[1], h->det_ev[2]));
        h->det_upload_ms = a;
        h->det_pipeline_ms = b;
        h->det_readback_ms = 0;
    }
    const unsigned long long *c = h->h_det_counts;
    if (dropped_blobs) *dropped_blobs = c[1];
    if (dropped_features) *dropped_features = c[4];
    const uint64_t n_kp = std::min<uint64_t>(c[3], max_out);
    if (n_kp == 0) return LF_MKD_OK;
    LF_HIP(h, hipMemcpyAsync(descriptors, h->d_det_desc, n_kp * kOut * 4, hipMemcpyDeviceToHost, s));
    std::memcpy(keypoints, h->h_res_kps, n_kp * sizeof(lf_mkd_keypoint));
    LF_HIP(h, hipStreamSynchronize(s));
    if (timed) h->det_readback_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_back).count();
    *n_out = n_kp;
    return LF_MKD_OK;
}

static int detect_host(lf_mkd *h, const float *image, const unsigned char *image_u8, uint32_t width, uint32_t height,
                       uint32_t top_n, float min_size, lf_mkd_keypoint *keypoints, float *descriptors, uint64_t max_out,
                       uint64_t *n_out, uint64_t *dropped_blobs, uint64_t *dropped_features) {
    // validate and clamp
    if (!h) return LF_MKD_ERR_BAD_ARG;
    if (!n_out) return fail(h, LF_MKD_ERR_BAD_ARG, "detect: n_out is null");
    *n_out = 0;
    if (dropped_blobs) *dropped_blobs = 0;
    if (dropped_features) *dropped_features = 0;
    if (max_out && (!keypoints || !descriptors)) return fail(h, LF_MKD_ERR_BAD_ARG, "detect: null output pointer");
    if (!image && !image_u8) return fail(h, LF_MKD_ERR_BAD_ARG, "detect: null image");
    if (!h->d_image || !h->d_pyr || width < 2 || height < 2 || width > h->params.max_image_width ||
        height > h->params.max_image_height)
        return fail(h, LF_MKD_ERR_BAD_ARG, "detect: image exceeds max_image_width/height given at creation");
    LF_ENTER(h);
    hipStream_t s = h->stream;
    const bool u8 = image_u8 != nullptr;
    const void *frame = u8 ? static_cast<const void *>(image_u8) : image;
    if (u8)
        if (int rc = ensure_u8_staging(h)) return rc;
    // An extremum yields at most 18 keypoints: a capacity beyond that bound sizes nothing -- not the result staging, not
    // the pinned keypoint rows a recording copies on every call, not the key of a recording.
    max_out = std::min<uint64_t>(max_out, std::min<uint64_t>(top_n ? top_n : h->max_extrema, h->max_extrema) *
                                              LF_MKD_MAX_ANGLES_PER_EXTREMUM);
    DetectKey key{width, height, top_n, 0, max_out, u8};
    std::memcpy(&key.min_size_bits, &min_size, 4);

    const DetectForm form = choose_form(h, key);
    if (form == DetectForm::stepwise) {
        h->det_upload_ms = h->det_pipeline_ms = h->det_readback_ms = 0;    // lf_mkd_detect_times covers recorded calls only
        if (int rc = upload_frame(h, frame, u8, width, height, nullptr)) return rc;
        return detect_stepwise(h, u8, width, height, top_n, min_size, keypoints, descriptors, max_out, n_out, dropped_blobs,
                               dropped_features);
    }
    // every buffer the recording names, before the upload is queued (growing one waits for the device)
    const uint64_t cap = top_n ? top_n : h->max_extrema;
    if (int rc = prepare_pipeline(h, top_n, cap)) return rc;
    if (int rc = ensure_orient_scratch(h, cap, true, max_out)) return rc;     // d_kps_out, d_det_desc [max_out]
    if (int rc = grow(h, h->h_res_kps, max_out)) return rc;
    if (!h->d_det_counts) {
        LF_HIP(h, h->d_det_counts.allocate(8));
        LF_HIP(h, hipMemsetAsync(h->d_det_counts, 0, 8 * sizeof(unsigned long long), s));
        LF_HIP(h, h->h_det_counts.allocate(8));
        LF_HIP(h, hipStreamSynchronize(s));
    }
    const bool timed = h->params.flags & LF_MKD_FLAG_KERNEL_TIMING;
    if (timed) {
        for (auto &e : h->det_ev)
            if (!e) LF_HIP(h, hipEventCreate(&e));
        LF_HIP(h, hipEventRecord(h->det_ev[0], s));
    }
    describe_pyramid(width, height, h->pd);

    // the recording (the buffers above may have moved and retired every recording: look again), or the plain launches' stream
    DetectPlan *plan = nullptr;
    if (form == DetectForm::recorded && !(plan = h->plans.find(key))) {
        if (int rc = h->plans.make_room([&] {
                LF_HIP(h, hipStreamSynchronize(s));
                return LF_MKD_OK;
            }))
            return rc;
        DetectPlan p;
        if (int rc = record_plan(h, key, min_size, p)) return rc;
        plan = &h->plans.add(key, std::move(p));
    }
    if (form == DetectForm::direct && h->pd.levels >= 2)
        if (int rc = ensure_side_stream(h, 2)) return rc;

    // upload, launch
    if (int rc = upload_frame(h, frame, u8, width, height, plan)) return rc;
    if (timed) LF_HIP(h, hipEventRecord(h->det_ev[1], s));     // (on s behind the last piece's wait: the whole frame is there)
    if (plan) {
        LF_HIP(h, hipGraphLaunch(plan->graph.exec, s));
    } else {
        enqueue_pipeline(h, width, height, top_n, min_size, max_out, u8 ? nullptr : h->d_image.get(),
                         u8 ? h->d_image_u8.get() : nullptr, h->d_kps_out, h->d_det_desc, h->d_det_counts, h->h_det_counts,
                         h->h_res_kps, nullptr);
        LF_HIP(h, hipGetLastError());
    }
    if (timed) LF_HIP(h, hipEventRecord(h->det_ev[2], s));
    h->n_frames = 1;
    h->have_image = h->coarse_valid = h->coarse_l1_valid = true;   // the handle holds this frame's pyramid and a-trous stack
    LF_HIP(h, hipStreamSynchronize(s));

    return read_back(h, timed, keypoints, descriptors, max_out, n_out, dropped_blobs, dropped_features);
}

int lf_mkd_detect_recordings(const lf_mkd *h, uint32_t *n_recordings, uint32_t *n_banded, uint32_t *n_sightings) {
    if (!h) return LF_MKD_ERR_BAD_ARG;
    uint32_t banded = 0;
    h->plans.for_each([&](const DetectPlan &p) { banded += p.cuts.empty() ? 0u : 1u; });
    if (n_recordings) *n_recordings = uint32_t(h->plans.size());
    if (n_banded) *n_banded = banded;
    if (n_sightings) *n_sightings = uint32_t(h->sightings.size());
    return LF_MKD_OK;
}

int lf_mkd_detect_times(lf_mkd *h, double *upload_ms, double *pipeline_ms, double *readback_ms) {
    if (!h) return LF_MKD_ERR_BAD_ARG;
    if (!(h->params.flags & LF_MKD_FLAG_KERNEL_TIMING))
        return fail(h, LF_MKD_ERR_BAD_ARG, "detect_times: the handle was not created with LF_MKD_FLAG_KERNEL_TIMING");
    if (upload_ms) *upload_ms = h->det_upload_ms;
    if (pipeline_ms) *pipeline_ms = h->det_pipeline_ms;
    if (readback_ms) *readback_ms = h->det_readback_ms;
    return LF_MKD_OK;
}

int lf_mkd_detect(lf_mkd *h, const float *image, uint32_t width, uint32_t height, uint32_t top_n, float min_size,
                  lf_mkd_keypoint *keypoints, float *descriptors, uint64_t max_out, uint64_t *n_out,
                  uint64_t *dropped_blobs, uint64_t *dropped_features) {
    if (h && !image) return fail(h, LF_MKD_ERR_BAD_ARG, "detect: null image");
    return detect_host(h, image, nullptr, width, height, top_n, min_size, keypoints, descriptors, max_out, n_out,
                       dropped_blobs, dropped_features);
}

int lf_mkd_detect_u8(lf_mkd *h, const uint8_t *image, uint32_t width, uint32_t height, uint32_t top_n, float min_size,
                     lf_mkd_keypoint *keypoints, float *descriptors, uint64_t max_out, uint64_t *n_out,
                     uint64_t *dropped_blobs, uint64_t *dropped_features) {
    if (h && !image) return fail(h, LF_MKD_ERR_BAD_ARG, "detect_u8: null image");
    return detect_host(h, nullptr, image, width, height, top_n, min_size, keypoints, descriptors, max_out, n_out,
                       dropped_blobs, dropped_features);
}

int lf_mkd_detect_frames_device(lf_mkd *h, const float *d_images, uint32_t n_frames, uint32_t width, uint32_t height,
                                uint32_t top_n, float min_size, lf_mkd_keypoint *d_keypoints, uint32_t *d_frame_of_kp,
                                float *d_descriptors, uint64_t max_out, uint64_t *n_out, uint64_t *dropped_blobs,
                                uint64_t *dropped_features, void *stream) {
    if (!h) return LF_MKD_ERR_BAD_ARG;
    if (!n_out) return fail(h, LF_MKD_ERR_BAD_ARG, "detect_frames: n_out is null");
    *n_out = 0;
    if (dropped_blobs) *dropped_blobs = 0;
    if (dropped_features) *dropped_features = 0;
    if (max_out && (!d_keypoints || !d_descriptors || !d_frame_of_kp))
        return fail(h, LF_MKD_ERR_BAD_ARG, "detect_frames: null output pointer");
    LF_ENTER(h);
    if (int rc = lf_mkd_set_images_device(h, d_images, n_frames, width, height, stream)) return rc;
    hipStream_t s = stream_of(h, stream);
    const uint64_t cap_f = h->max_extrema;                       // extrema kept per frame (mod.rs:625-633)
    const uint64_t keep = top_n ? std::min<uint64_t>(top_n, cap_f) : cap_f;
    // the batch's extremum list: cap_f rows per frame, each frame's share its own (a frame with more than cap_f extrema
    // loses the ones beyond them, as lf_mkd_detect does, and takes nothing from the other frames)
    const uint64_t all_cap = cap_f * n_frames;
    if (all_cap > 0xFFFFFFFFull) return fail(h, LF_MKD_ERR_BAD_ARG, "detect_frames: max_blobs x frames exceeds 2^32");
    if (int rc = ensure_coarse_stack(h, s)) return rc;
    if (int rc = ensure_detect_scratch(h)) return rc;
    if (int rc = grow(h, h->d_det_extrema, all_cap)) return rc;
    if (int rc = grow(h, h->d_mf_frame_count, n_frames)) return rc;
    if (int rc = grow(h, h->d_mf_offsets, n_frames)) return rc;
    if (int rc = grow(h, h->d_mf_padded, keep * n_frames)) return rc;
    if (int rc = grow(h, h->d_mf_list, keep * n_frames)) return rc;
    if (int rc = grow(h, h->d_mf_frame_of, keep * n_frames)) return rc;
    // 1. every frame's extrema, ordered by frame; 2. per-frame selection; 3. one contiguous list + frame ids
    launch_detect_extrema(h->d_pyr + h->pd.offset[0], h->pyr_stride, h->pd.pitch[0], h->d_coarse, h->coarse_stride, h->layer_stride,
                          h->n_layers, int(width), int(height), int(n_frames), kBorder, kSkipLayers, kContrastThreshold,
                          h->d_slots, h->d_cube_counts, h->d_cube_sums, h->d_det_extrema.as<float>(), nullptr, h->d_mf_frame_count,
                          cap_f, nullptr, s);
    launch_topk_filter(h->d_det_extrema.as<float>(), h->d_mf_frame_count, nullptr, 0, n_frames, unsigned(cap_f),
                       unsigned(keep), top_n ? min_size : -INFINITY, h->d_mf_padded.as<float>(), nullptr, h->d_sel_count,
                       nullptr, 0, nullptr, s);
    launch_segments_compact(h->d_mf_padded.as<float>(), h->d_sel_count, h->d_mf_frame_count, n_frames, unsigned(cap_f),
                            unsigned(keep), h->d_mf_offsets, h->d_mf_list.as<float>(), h->d_mf_frame_of, h->d_totals + 0, s);
    LF_HIP(h, hipGetLastError());
    unsigned long long totals[2] = {0, 0};
    LF_HIP(h, hipMemcpyAsync(totals, h->d_totals, sizeof(totals), hipMemcpyDeviceToHost, s));
    LF_HIP(h, hipStreamSynchronize(s));
    const uint64_t n_sel = totals[0];
    if (dropped_blobs) *dropped_blobs = totals[1];
    if (n_sel == 0 || max_out == 0) return LF_MKD_OK;
    // 4. orientation over the whole list, 5. sampling + description by frame id
    if (int rc = ensure_orient_scratch(h, n_sel, false, 0)) return rc;
    uint64_t n_kp = 0;
    if (int rc = orient_device(h, h->d_mf_list.as<float>(), h->d_mf_frame_of, n_sel, reinterpret_cast<float *>(d_keypoints),
                               d_frame_of_kp, max_out, &n_kp, dropped_features, s))
        return rc;
    *n_out = n_kp;
    if (n_kp == 0) return LF_MKD_OK;
    return lf_mkd_describe_keypoints_frames_device(h, d_keypoints, d_frame_of_kp, n_kp, d_descriptors, s);
}

int lf_mkd_stream_create(lf_mkd *h, uint32_t width, uint32_t height, uint32_t top_n, float min_size, uint64_t max_out,
                         const float *d_image, lf_mkd_keypoint *d_keypoints, float *d_descriptors, uint64_t *d_counts) {
    if (!h) return LF_MKD_ERR_BAD_ARG;
    if (!d_image || !d_keypoints || !d_descriptors || !d_counts || max_out == 0 || width < 2 || height < 2)
        return fail(h, LF_MKD_ERR_BAD_ARG, "stream_create: bad argument");
    if (!h->d_pyr || width > h->params.max_image_width || height > h->params.max_image_height)
        return fail(h, LF_MKD_ERR_BAD_ARG, "stream_create: frame exceeds max_image_width/height given at creation");
    LF_ENTER(h);
    LF_HIP(h, hipStreamSynchronize(h->stream));
    // an earlier recording may still be running on a caller's stream
    if (h->stream_graph) {
        (void)hipDeviceSynchronize();
        h->stream_graph.reset();
    }
    // every allocation happens before the capture starts
    describe_pyramid(width, height, h->pd);
    h->n_frames = 1;
    // no frame has gone through the recorded pipeline yet: until lf_mkd_stream_frame runs, the pyramid and the a-trous
    // stack hold nothing the keypoint / orientation / verification entry points could use
    h->have_image = false;
    h->coarse_valid = h->coarse_l1_valid = false;
    const uint64_t cap = top_n ? top_n : h->max_extrema;   // extrema that can reach orientation
    if (int rc = prepare_pipeline(h, top_n, cap)) return rc;
    if (!fused_keypoints(h))
        if (int rc = grow(h, h->d_stream_patches, max_out * kPx)) return rc;
    unsigned long long *cnt = reinterpret_cast<unsigned long long *>(d_counts);
    LF_HIP(h, hipMemsetAsync(cnt, 0, 8 * sizeof(unsigned long long), h->stream));
    LF_HIP(h, hipStreamSynchronize(h->stream));
    if (int rc = record_pipeline(h, width, height, top_n, min_size, max_out, d_image, nullptr, d_keypoints, d_descriptors, cnt,
                                 nullptr, nullptr, h->stream_graph))
        return rc;
    h->graph_pd = h->pd;
    return LF_MKD_OK;
}

int lf_mkd_stream_frame(lf_mkd *h, void *stream) {
    if (!h) return LF_MKD_ERR_BAD_ARG;
    if (!h->stream_graph)
        return fail(h, LF_MKD_ERR_BAD_ARG, "stream_frame: no recorded pipeline (call lf_mkd_stream_create; a call that "
                                           "grew the handle's scratch buffers retires an earlier recording)");
    LF_ENTER(h);
    LF_HIP(h, hipGraphLaunch(h->stream_graph.exec, stream_of(h, stream)));
    // every launch rebuilds the pyramid and the a-trous stack of the frame in d_image: work enqueued behind it on the same
    // stream (describe_keypoints, orientation, the verification taps) sees that frame
    h->pd = h->graph_pd;
    h->n_frames = 1;
    h->have_image = h->coarse_valid = h->coarse_l1_valid = true;
    return LF_MKD_OK;
}

int lf_mkd_orient_keypoints_blocked(lf_mkd *h, const float *extremum_data, uint64_t n_extrema, uint32_t block_len,
                                    const uint32_t *indices, uint64_t n_indices, uint32_t *kp_extremum_index,
                                    float *kp_orientation, lf_mkd_keypoint *keypoints, uint64_t max_out, uint64_t *n_out,
                                    uint64_t *n_dropped) {
    if (!h) return LF_MKD_ERR_BAD_ARG;
    if (!n_out) return fail(h, LF_MKD_ERR_BAD_ARG, "orient_keypoints_blocked: n_out is null");
    *n_out = 0;
    if (n_dropped) *n_dropped = 0;
    if (n_indices == 0) return LF_MKD_OK;
    if (!extremum_data || !indices || block_len == 0 || (max_out && (!kp_extremum_index || !kp_orientation)))
        return fail(h, LF_MKD_ERR_BAD_ARG, "orient_keypoints_blocked: null pointer");
    // gather the blocked coordinate arrays into records (BlobLocations::get, shaders.rs:307-318)
    std::vector<lf_mkd_extremum> ex(n_indices);
    for (uint64_t i = 0; i < n_indices; ++i) {
        const uint64_t idx = indices[i];
        if (idx >= n_extrema) return fail(h, LF_MKD_ERR_BAD_ARG, "orient_keypoints_blocked: index beyond n_extrema");
        const uint64_t base = idx / block_len * 4 * block_len, off = idx % block_len;
        ex[i] = lf_mkd_extremum{extremum_data[base + off], extremum_data[base + block_len + off],
                                extremum_data[base + 2 * block_len + off], extremum_data[base + 3 * block_len + off]};
    }
    std::vector<lf_mkd_keypoint> kps(max_out);
    if (int rc = lf_mkd_orient_keypoints(h, ex.data(), n_indices, kps.data(), max_out, n_out, n_dropped)) return rc;
    // keypoints come ordered by extremum: walk both lists together to recover each keypoint's extremum
    uint64_t j = 0;
    for (uint64_t i = 0; i < *n_out; ++i) {
        while (j < n_indices && !(ex[j].x == kps[i].x && ex[j].y == kps[i].y && ex[j].size == kps[i].size &&
                                  ex[j].response == kps[i].response))
            ++j;
        if (j == n_indices) return fail(h, LF_MKD_ERR_HIP, "orient_keypoints_blocked: keypoint without an extremum");
        kp_extremum_index[i] = indices[j];
        kp_orientation[i] = kps[i].angle;
        if (keypoints) keypoints[i] = kps[i];
    }
    return LF_MKD_OK;
}

int lf_mkd_get_coarse_layer(lf_mkd *h, uint32_t layer, float *out) {
    if (!h) return LF_MKD_ERR_BAD_ARG;
    if (!h->have_image) return fail(h, LF_MKD_ERR_NO_IMAGE, "get_coarse_layer: call lf_mkd_set_image first");
    if (layer >= uint32_t(h->n_layers) || !out) return fail(h, LF_MKD_ERR_BAD_ARG, "get_coarse_layer: bad layer");
    LF_ENTER(h);
    if (int rc = ensure_coarse_stack(h, h->stream)) return rc;
    LF_HIP(h, hipStreamSynchronize(h->stream));
    const float *src = layer == 0 ? h->d_pyr + h->pd.offset[0] : h->d_coarse + long(layer - 1) * h->layer_stride;
    const size_t spitch = size_t(layer == 0 ? h->pd.pitch[0] : h->pd.w[0]) * 4;
    LF_HIP(h, hipMemcpy2D(out, size_t(h->pd.w[0]) * 4, src, spitch, size_t(h->pd.w[0]) * 4, size_t(h->pd.h[0]),
                          hipMemcpyDeviceToHost));
    return LF_MKD_OK;
}

int lf_mkd_get_pyramid_level(lf_mkd *h, uint32_t level, float *out, uint32_t *w, uint32_t *hgt) {
    if (!h) return LF_MKD_ERR_BAD_ARG;
    if (!h->have_image) return fail(h, LF_MKD_ERR_NO_IMAGE, "get_pyramid_level: call lf_mkd_set_image first");
    if (level >= uint32_t(h->pd.levels)) return fail(h, LF_MKD_ERR_BAD_ARG, "get_pyramid_level: no such level");
    if (w) *w = uint32_t(h->pd.w[level]);
    if (hgt) *hgt = uint32_t(h->pd.h[level]);
    if (!out) return LF_MKD_OK;
    LF_ENTER(h);
    LF_HIP(h, hipStreamSynchronize(h->stream));
    LF_HIP(h, hipMemcpy2D(out, size_t(h->pd.w[level]) * 4, h->d_pyr + h->pd.offset[level], size_t(h->pd.pitch[level]) * 4,
                          size_t(h->pd.w[level]) * 4, size_t(h->pd.h[level]), hipMemcpyDeviceToHost));
    return LF_MKD_OK;
}

int lf_mkd_get_pyramid_level_apron(lf_mkd *h, uint32_t level, float *out, uint32_t *w, uint32_t *hgt, uint32_t *apron) {
    if (!h) return LF_MKD_ERR_BAD_ARG;
    if (!h->have_image) return fail(h, LF_MKD_ERR_NO_IMAGE, "get_pyramid_level_apron: call lf_mkd_set_image first");
    if (level >= uint32_t(h->pd.levels)) return fail(h, LF_MKD_ERR_BAD_ARG, "get_pyramid_level_apron: no such level");
    const int a = h->pd.apron[level], pw = h->pd.w[level] + 2 * a, ph = h->pd.h[level] + 2 * a;
    if (w) *w = uint32_t(h->pd.w[level]);
    if (hgt) *hgt = uint32_t(h->pd.h[level]);
    if (apron) *apron = uint32_t(a);
    if (!out) return LF_MKD_OK;
    LF_ENTER(h);
    LF_HIP(h, hipStreamSynchronize(h->stream));
    const float *src = h->d_pyr + h->pd.offset[level] - long(a) * h->pd.pitch[level] - a;
    LF_HIP(h, hipMemcpy2D(out, size_t(pw) * 4, src, size_t(h->pd.pitch[level]) * 4, size_t(pw) * 4, size_t(ph),
                          hipMemcpyDeviceToHost));
    return LF_MKD_OK;
}

}  // extern "C"
