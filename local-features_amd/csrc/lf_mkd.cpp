// C ABI of the MKD path (include/lf_mkd.h): handle management, batching, host<->device staging.
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

#include "lf_mkd_internal.h"
#include "mkd_consts.hpp"
#include "mkd_device.h"

using namespace lfmkd;

namespace {

enum Memory { kDevice, kPinned };

// An array of T in device (or pinned host) memory and the elements it holds; freed when its owner goes.
// Recorded: a recorded pipeline names the array by address and the array can grow while a recording exists, so allocating
// it retires every recording first (grow).  An array a recording reads that is allocated once, at its final size, is not.
template <typename T, Memory M = kDevice, bool Recorded = false>
class HipArray {
  public:
    HipArray() = default;
    HipArray(HipArray &&o) noexcept : p_(std::exchange(o.p_, nullptr)), cap_(std::exchange(o.cap_, 0)) {}
    HipArray &operator=(HipArray &&o) noexcept {
        std::swap(p_, o.p_);
        std::swap(cap_, o.cap_);
        return *this;
    }
    ~HipArray() { reset(); }
    operator T *() const { return p_; }
    T *get() const { return p_; }
    template <typename U>
    U *as() const { return reinterpret_cast<U *>(p_); }
    uint64_t cap() const { return cap_; }
    void reset() {
        if (p_) (void)(M == kPinned ? hipHostFree(p_) : hipFree(p_));
        p_ = nullptr;
        cap_ = 0;
    }
    // frees what the array holds, then room for max(n, 1) elements; cap() is n once that succeeded
    hipError_t allocate(uint64_t n) {
        reset();
        void *p = nullptr;
        const size_t bytes = std::max<uint64_t>(n, 1) * sizeof(T);
        const hipError_t e = M == kPinned ? hipHostMalloc(&p, bytes, hipHostMallocDefault) : hipMalloc(&p, bytes);
        if (e != hipSuccess) return e;
        p_ = static_cast<T *>(p);
        cap_ = n;
        return hipSuccess;
    }

  private:
    T *p_ = nullptr;
    uint64_t cap_ = 0;
};
template <typename T, Memory M = kDevice>
using RecordedArray = HipArray<T, M, true>;

// An instantiated recording.  Whoever drops one that may still be running waits for the device first.
struct Recording {
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    Recording() = default;
    Recording(Recording &&o) noexcept : graph(std::exchange(o.graph, nullptr)), exec(std::exchange(o.exec, nullptr)) {}
    Recording &operator=(Recording &&o) noexcept {
        std::swap(graph, o.graph);
        std::swap(exec, o.exec);
        return *this;
    }
    ~Recording() { reset(); }
    void reset() {
        if (exec) (void)hipGraphExecDestroy(exec);
        if (graph) (void)hipGraphDestroy(graph);
        exec = nullptr;
        graph = nullptr;
    }
    explicit operator bool() const { return exec != nullptr; }
};

// A request of lf_mkd_detect / lf_mkd_detect_u8: what a recording of its pipeline is specific to
struct DetectKey {
    uint32_t w, h, top_n, min_size_bits;
    uint64_t max_out;
    bool u8;
    bool operator==(const DetectKey &o) const {
        return w == o.w && h == o.h && top_n == o.top_n && min_size_bits == o.min_size_bits && max_out == o.max_out && u8 == o.u8;
    }
};

// At most Cap values by request; the least recently found or added one makes room for a new request.
template <typename V, size_t Cap>
class LruList {
  public:
    V *find(const DetectKey &key) {
        for (Entry &e : items_)
            if (e.key == key) {
                e.stamp = ++clock_;
                return &e.value;
            }
        return nullptr;
    }
    // Room for one more: when the list is full, before_drop() runs and then the least recently used entry goes (a nonzero
    // code from before_drop is returned, and the entry stays).
    template <typename F>
    int make_room(F before_drop) {
        if (items_.size() < Cap) return 0;
        auto old = std::min_element(items_.begin(), items_.end(), [](const Entry &a, const Entry &b) { return a.stamp < b.stamp; });
        if (int rc = before_drop()) return rc;
        items_.erase(old);
        return 0;
    }
    V &add(const DetectKey &key, V value) {
        items_.push_back(Entry{key, std::move(value), ++clock_});
        return items_.back().value;
    }
    void clear() { items_.clear(); }
    size_t size() const { return items_.size(); }
    template <typename F>
    void for_each(F f) const {
        for (const Entry &e : items_) f(e.value);
    }

  private:
    struct Entry {
        DetectKey key;
        V value;
        uint64_t stamp;
    };
    std::vector<Entry> items_;
    uint64_t clock_ = 0;
};

// lf_mkd_detect's recording of one request.  Banded form (frames large enough to be worth it): the frame is uploaded in
// pieces, rows [0, cuts[0]) first, then [cuts[0], cuts[1]) ...; heads[p] is the share of the pipeline's front the frame's
// first cuts[p] rows allow beyond heads[p - 1]'s (RowBands) and runs while piece p + 1 is on its way, `graph` is then the
// last piece's share + everything else
struct DetectPlan {
    Recording graph;
    std::vector<uint32_t> cuts;
    std::vector<Recording> heads;
};

}  // namespace

struct lf_mkd {
    lf_mkd_params params{};
    hipStream_t stream = nullptr;
    hipStream_t side_stream = nullptr;   // lf_mkd_detect / the recorded pipeline: pyramid levels >= 1 are built here beside the detector
    std::vector<hipEvent_t> side_events;
    struct {                             // the model's constants, uploaded at creation ...
        HipArray<short> colmap, colmap_unfolded;
        HipArray<float> pool_b_f32, white_a_f32, white_bias, odd_cart;
        HipArray<uint16_t> pool_b_f16, pool_b_fp6, white_a_f16, white_a_f16_unfolded;
    } consts;
    DeviceConsts dc;                     // ... as the launchers take them
    uint64_t batch = 0;                  // descriptors per internal batch (multiple of 64)
    HipArray<float> d_patches;           // [batch][1024] staging: host patches / sampled patches
    HipArray<float> d_out;               // [batch][128]  staging for host output
    HipArray<float> d_kps;               // [batch][5]
    // keypoint mode
    PyramidDesc pd{};
    HipArray<float> d_image, d_pyr, d_tmp_a, d_tmp_b;
    bool have_image = false;
    uint32_t max_frames = 1, n_frames = 0;  // frames held by the pyramid store / currently loaded
    long pyr_stride = 0;                    // floats between the pyramids of consecutive frames
    // keypoint orientation: a-trous layers 1 .. n_layers-1 per frame (layer 0 = pyramid level 0), allocated on first use
    int n_layers = 7;
    HipArray<float> d_coarse;
    long layer_stride = 0, coarse_stride = 0;  // floats between layers / between frames
    bool coarse_valid = false, coarse_l1_valid = false;
    // orientation scratch for max(n, batch) extrema, and the keypoint rows of lf_mkd_orient_keypoints / lf_mkd_detect
    RecordedArray<lf_mkd_extremum> d_extrema;
    RecordedArray<float> d_angles;
    RecordedArray<unsigned> d_counts, d_orient_sums;
    RecordedArray<lf_mkd_keypoint> d_kps_out;
    RecordedArray<float> d_det_desc;           // [max_out][128] lf_mkd_detect's descriptor staging
    HipArray<unsigned long long> d_totals;
    HipArray<unsigned long long> d_clk;        // LF_MKD_FLAG_KERNEL_TIMING: clock stamps of the latest describe launch
    // Claim counters of the patch-mode describe launches (launch_describe): a ring, one 64-byte line per slot, a slot per
    // launch in turn.  A launch clears its own slot on its own stream, so nothing is left over from the launch before; the
    // ring keeps launches of one handle that overlap on different streams (up to kClaimSlots of them) on different words.
    // A recorded pipeline keeps the slot it was recorded with: its replays are ordered on one stream.
    static constexpr unsigned kClaimSlots = 16, kClaimStride = 16;
    HipArray<unsigned> d_claims;
    unsigned claim_turn = 0;
    unsigned *next_claim() { return d_claims.get() + kClaimStride * (claim_turn++ % kClaimSlots); }
    // the row-split form of the keypoint kernel (requests of at most 16 x CUs keypoints): partial sums and their counters
    HipArray<float> d_kp_xchg;
    HipArray<unsigned> d_kp_words;
    // detector scratch (allocated on first use): per-cube slots and counts for max_frames frames of the maximum size
    uint64_t max_extrema = 8192;
    HipArray<float> d_slots;
    HipArray<unsigned> d_cube_counts, d_cube_sums, d_sel_count;
    RecordedArray<lf_mkd_extremum> d_det_extrema, d_det_selected;
    RecordedArray<unsigned> d_topk_work;
    // multi-frame detect (lf_mkd_detect_frames_device)
    HipArray<lf_mkd_extremum> d_mf_padded, d_mf_list;
    HipArray<unsigned> d_mf_frame_count, d_mf_offsets, d_mf_frame_of;
    // graph-captured per-frame pipeline (lf_mkd_stream_*)
    PyramidDesc graph_pd{};     // frame geometry the recorded pipeline was captured for
    RecordedArray<float> d_stream_patches;
    // lf_mkd_detect / lf_mkd_detect_u8: the same launch sequence recorded once per request (DetectKey) and kept -- a call is
    // one upload, one graph launch, one wait, the result copies.
    // Requests seen but not recorded yet.  Recording costs a capture and an instantiation (more when the upload is banded) --
    // several times the call itself -- so a request is served by the pipeline's plain launches until it has been seen record_after times
    // (default 1: the reference's match_images detects each image once, at its own size, and never pays a recording; a
    // camera loop records on its second frame and replays from the third).  LF_MKD_DETECT_RECORD_AFTER in the environment,
    // read at creation: 0 records on the first sighting.
    uint64_t record_after = 1;
    HipArray<unsigned char> d_image_u8;               // 8-bit frame(s) on their way to level 0, allocated on first use
    HipArray<unsigned long long> d_det_counts;        // [8] the recorded detect pipeline's counts (as lf_mkd_stream_create's d_counts)
    HipArray<unsigned long long, kPinned> h_det_counts;   // the same in pinned host memory: the last node of a plan copies them here
    // ... and the keypoints, copied there by the pipeline's last node.
    // (The descriptors stay in device memory until the count is known: having the describe kernel store them straight into
    // pinned host memory was measured -- +20 us of kernel time at 100 keypoints, +45 us at 3000, PCIe writes stall its
    // epilogue -- and so was a copy node of all max_out rows followed by a host memcpy of n: reading memory the device has
    // just written runs at 25 GB/s on one core, 60 us for 3000 rows, where the runtime's own copy into the caller's array takes 15.)
    RecordedArray<lf_mkd_keypoint, kPinned> h_res_kps;
    hipStream_t copy_stream = nullptr;                    // the banded upload: pieces are copied here, the pipeline's parts wait for them
    std::vector<hipEvent_t> copy_ev;
    hipEvent_t det_ev[3] = {nullptr, nullptr, nullptr};   // LF_MKD_FLAG_KERNEL_TIMING: before the upload, after it, after the pipeline
    double det_upload_ms = 0, det_pipeline_ms = 0, det_readback_ms = 0;
    // matcher scratch
    HipArray<unsigned char> d_match_a, d_match_b;
    HipArray<float> d_match_part, d_match_in;
    HipArray<int> d_match_out;
    HipArray<unsigned char> d_match_rec;       // two-pass form: candidate records, their counts, |a| per row, two words
    HipArray<unsigned char> d_match_cnt;       // (largest |b| as float bits, number of overflowed rows)
    HipArray<float> d_match_norm, d_match_floor;   // (floor: the bounds the screen's b splits share, per a row)
    HipArray<unsigned> d_match_misc;
    HipArray<unsigned char> d_match_few_tiles;   // the overflowed rows' own tiles; their indices, exclusion ranges, partials
    HipArray<unsigned> d_match_few;
    // 8-bit descriptors: the int8 matcher's per-split partials (match_q8_plan's scratch_bytes), and the host forms' staging
    HipArray<unsigned char> d_q8_part, d_q8_io;
    // RANSAC verification scratch (lf_mkd_verify_homography*, lf_mkd_verify_fundamental*, which share it): per-pair
    // normalisation, per-candidate partial counts, and the host form's staging.  No recording names them; they grow only when a call asks for more, so the device form's launches
    // can be captured once warmed up.  Calls of one handle are stream-ordered (lf_mkd.h).
    // lf_mkd_track_table_device's scratch (track_table_plan's scratch_bytes); like the verifiers' it is named by no recording
    HipArray<unsigned char> d_track_table;
    // lf_mkd_link_table_device's scratch (link_table_plan's scratch_bytes), in the same way
    HipArray<unsigned char> d_link_table;
    // lf_mkd_select_edges_device's scratch (select_edges_plan's scratch_bytes), in the same way
    HipArray<unsigned char> d_select_edges;
    // lf_mkd_covisibility_device's scratch (covisibility_plan's scratch_bytes), in the same way
    HipArray<unsigned char> d_covisibility;
    // lf_mkd_resect_cameras_device's scratch (resect_scratch_bytes), in the same way
    HipArray<unsigned char> d_resect;
    HipArray<VerifyPair> d_ver_pairs;
    HipArray<unsigned> d_ver_counts;
    HipArray<unsigned char> d_ver_io;
    int num_cus = 256;
    // LF_MKD_FLAG_KERNEL_TIMING: (start, end) of the describe kernel per batch
    std::vector<hipEvent_t> ev_pending, ev_free;
    std::string err;
    // The recordings, declared after every array they name: they are destroyed first.
    Recording stream_graph;              // lf_mkd_stream_*
    LruList<DetectPlan, 8> plans;        // lf_mkd_detect's recordings
    LruList<uint64_t, 64> sightings;     // times a request not recorded yet was served by the plain launches
};

namespace {

thread_local std::string g_create_error;

#define LF_HIP(h, call)                                                                     \
    do {                                                                                    \
        hipError_t e_ = (call);                                                             \
        if (e_ != hipSuccess) {                                                             \
            (h)->err = std::string(#call) + ": " + hipGetErrorString(e_);                   \
            return LF_MKD_ERR_HIP;                                                          \
        }                                                                                   \
    } while (0)

// Every entry point makes the handle's device current for its own duration and puts the caller's device back on EVERY return
// path (a one-process / one-handle-per-GPU caller -- INTEGRATION.md section 3 -- keeps the current device it had).
#define LF_ENTER(h)              \
    lfmkd::DeviceScope scope_;   \
    LF_HIP(h, scope_.enter((h)->params.device))

int fail(lf_mkd *h, int code, const std::string &msg) {
    if (h) h->err = msg;
    return code;
}

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

// A recorded pipeline holds raw pointers into the scratch buffers: re-allocating one of them retires the recordings
// (lf_mkd_stream_frame then asks for a new lf_mkd_stream_create instead of touching freed memory, and lf_mkd_detect records anew).
void retire_graph(lf_mkd *h) {
    if (h->stream_graph || h->plans.size()) (void)hipDeviceSynchronize();   // a launch may still be running (on any stream)
    h->stream_graph.reset();
    h->plans.clear();
}

// The one growth path of the handle's arrays: an array that holds fewer than `want` elements (or none) is freed, then
// allocated for max(want, 1).  Growing a Recorded array retires every recording first; growing any other (the matcher's and
// the multi-frame detect's scratch, say) leaves the recordings alone and does not wait for the device.
template <typename T, Memory M, bool Recorded>
int grow(lf_mkd *h, HipArray<T, M, Recorded> &buf, uint64_t want) {
    if (want <= buf.cap() && buf.get()) return LF_MKD_OK;
    if (Recorded) retire_graph(h);
    LF_HIP(h, buf.allocate(want));
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

constexpr uint64_t kMatchChunk = 1 << 20;   // a rows per pass of the two-pass matcher (2 GiB of records at one b split)

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

// the matcher's three words -- [0] largest |b| (float bits), [1] rows of the current chunk whose candidate records
// overflowed, [2] the same over the call (lf_mkd_match_overflowed) -- allocated on first use and zeroed once, on the stream
// the match will run on (so that a form that does not reset [2] adds to a defined value)
int ensure_match_misc(lf_mkd *h, hipStream_t s) {
    if (h->d_match_misc) return LF_MKD_OK;
    if (int rc = grow(h, h->d_match_misc, 3)) return rc;
    LF_HIP(h, hipMemsetAsync(h->d_match_misc, 0, 3 * sizeof(unsigned), s));
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
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : h->stream;
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
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : h->stream;
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
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : h->stream;
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
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : h->stream;
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
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : h->stream;
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
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : h->stream;
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
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : h->stream;
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
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : h->stream;
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
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : h->stream;
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
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : h->stream;
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
    LF_HIP(h, hipGraphLaunch(h->stream_graph.exec, stream ? static_cast<hipStream_t>(stream) : h->stream));
    // every launch rebuilds the pyramid and the a-trous stack of the frame in d_image: work enqueued behind it on the same
    // stream (describe_keypoints, orientation, the verification taps) sees that frame
    h->pd = h->graph_pd;
    h->n_frames = 1;
    h->have_image = h->coarse_valid = h->coarse_l1_valid = true;
    return LF_MKD_OK;
}

// keep_overflow: the word lf_mkd_match_overflowed reads is added to, not reset (the second direction of lf_mkd_match_both_device)
static int match_device_impl(lf_mkd *h, const float *d_a, uint64_t na, const float *d_b, uint64_t nb,
                             const uint32_t *d_exclude_lo, const uint32_t *d_exclude_hi, float ratio, int32_t *d_match,
                             float *d_best, float *d_second, void *stream, bool keep_overflow) {
    if (!h) return LF_MKD_ERR_BAD_ARG;
    if (na == 0) return LF_MKD_OK;
    if (!d_a || !d_b || !d_match) return fail(h, LF_MKD_ERR_BAD_ARG, "match_device: null pointer");
    if (nb < 2) return fail(h, LF_MKD_ERR_BAD_ARG, "match: needs at least two candidates in b (main.rs:20)");
    if ((d_exclude_lo == nullptr) != (d_exclude_hi == nullptr))
        return fail(h, LF_MKD_ERR_BAD_ARG, "match_device: exclude_lo and exclude_hi go together");
    if (na > 0x7FFFFFFFull || nb > 0x7FFFFFFFull) return fail(h, LF_MKD_ERR_BAD_ARG, "match: more than 2^31 rows");
    if ((reinterpret_cast<uintptr_t>(d_a) | reinterpret_cast<uintptr_t>(d_b)) & 15)
        return fail(h, LF_MKD_ERR_BAD_ARG, "match_device: d_a and d_b must be 16-byte aligned");
    LF_ENTER(h);
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : h->stream;
    // Which form: the two passes win once the scan would take about a millisecond and a has enough rows to fill the chip
    // without splitting b many ways (every b split starts its candidate lists from nothing); below that -- the reference's
    // own 2000 x 2000 included -- the three-term scan alone is faster.  LF_MKD_MATCH=scan / =screen in the environment
    // force one form (A/B runs, tests).
    // Small problems -- the reference's own 2000 x 2000 (examples/match_images/src/main.rs:62-76) -- take ONE launch that
    // reads the f32 rows directly (match_small: no operand tiles, no partials, no merge kernel): below ~10^4 rows the chain
    // of split / scan / merge launches is launch cadence, not arithmetic.  LF_MKD_MATCH=small forces it where it fits.
    const char *form = getenv("LF_MKD_MATCH");
    const bool want_small = form ? (form[0] == 's' && form[1] == 'm') : true;
    if (want_small && match_small_fits(long(na), long(nb))) {
        launch_match_small(d_a, long(na), d_b, long(nb), d_exclude_lo, d_exclude_hi, ratio, d_match, d_best, d_second,
                           h->d_match_misc && !keep_overflow ? h->d_match_misc + 2 : nullptr, s);
        LF_HIP(h, hipGetLastError());
        return LF_MKD_OK;
    }
    // (=small where it does not fit: the scan, as include/lf_mkd.h says -- never silently the two-pass form)
    const bool force_scan = form && ((form[0] == 's' && form[1] == 'c' && form[2] == 'a') || (form[0] == 's' && form[1] == 'm'));
    const bool three_term_only = force_scan ? true
                                            : (form && form[0] == 's' && form[1] == 'c' ? false : !(na >= 16384 && na * nb >= (1ull << 29)));
    // a goes through in chunks, so that the per-row scratch (2 KiB of candidate records per a row and b split) stays bounded
    const uint64_t chunk = three_term_only ? na : std::min<uint64_t>(na, kMatchChunk);
    const int splits = match_splits(long(chunk), long(nb), h->num_cus);
    if (int rc = grow(h, h->d_match_a, match_tiles_bytes(long(chunk)))) return rc;
    if (int rc = grow(h, h->d_match_b, match_tiles_bytes(long(nb)))) return rc;
    if (int rc = grow(h, h->d_match_part, uint64_t(splits) * chunk * 3)) return rc;
    float *p_best = h->d_match_part, *p_second = p_best + uint64_t(splits) * chunk;
    int *p_index = reinterpret_cast<int *>(p_second + uint64_t(splits) * chunk);
    if (three_term_only) {
        // lf_mkd_match_overflowed reports on the LATEST call: this form redoes nothing
        if (h->d_match_misc && !keep_overflow) LF_HIP(h, hipMemsetAsync(h->d_match_misc + 2, 0, sizeof(unsigned), s));
        launch_match_split(d_a, long(na), h->d_match_a, nullptr, nullptr, s);
        launch_match_split(d_b, long(nb), h->d_match_b, nullptr, nullptr, s);
        launch_match(h->d_match_a, long(na), h->d_match_b, long(nb), d_exclude_lo, d_exclude_hi, ratio, splits, p_best,
                     p_index, p_second, d_match, d_best, d_second, nullptr, s);
        LF_HIP(h, hipGetLastError());
        return LF_MKD_OK;
    }
    if (int rc = grow(h, h->d_match_rec, match_record_bytes(long(chunk), splits))) return rc;
    if (int rc = grow(h, h->d_match_cnt, match_count_bytes(long(chunk), splits))) return rc;
    if (int rc = grow(h, h->d_match_norm, chunk)) return rc;
    if (int rc = grow(h, h->d_match_floor, chunk)) return rc;   // the splits' shared bounds
    if (int rc = ensure_match_misc(h, s)) return rc;
    if (int rc = grow(h, h->d_match_few_tiles, match_few_tiles_bytes())) return rc;
    if (int rc = grow(h, h->d_match_few, match_few_words())) return rc;
    // misc: [0] largest |b| (float bits), [1] rows of the current chunk whose records overflowed, [2] the same over the call
    LF_HIP(h, hipMemsetAsync(h->d_match_misc, 0, (keep_overflow ? 2 : 3) * sizeof(unsigned), s));
    unsigned *b_max = h->d_match_misc;
    int *n_over = reinterpret_cast<int *>(h->d_match_misc + 1);
    launch_match_split(d_b, long(nb), h->d_match_b, nullptr, b_max, s);
    for (uint64_t at = 0; at < na; at += chunk) {
        const long n = long(std::min(chunk, na - at));
        const float *a = d_a + at * kOut;
        const uint32_t *lo = d_exclude_lo ? d_exclude_lo + at : nullptr, *hi = d_exclude_hi ? d_exclude_hi + at : nullptr;
        float *best = d_best ? d_best + at : nullptr, *second = d_second ? d_second + at : nullptr;
        if (at) LF_HIP(h, hipMemsetAsync(n_over, 0, sizeof(int), s));
        launch_match_split(a, n, h->d_match_a, h->d_match_norm, nullptr, s);
        launch_match_screen(h->d_match_a, n, h->d_match_b, long(nb), lo, hi, splits, h->d_match_norm, b_max,
                            h->d_match_rec, h->d_match_cnt, s, h->d_match_floor.as<int>());
        launch_match_verify(a, n, d_b, h->d_match_norm, b_max, h->d_match_rec, h->d_match_cnt, splits, ratio,
                            d_match + at, best, second, n_over, h->d_match_few.as<int>(), s);
        // rows whose records overflowed (more than 64 near-best candidates in one lane's share of b) are redone by the
        // three-term scan: on their own when they are few, else the whole chunk; both are enqueued unconditionally and
        // read the count on the device -- no host round trip, and nothing to do in the ordinary case
        launch_match_few(a, h->d_match_b, long(nb), lo, hi, ratio, n_over, h->d_match_few_tiles, h->d_match_few,
                         d_match + at, best, second, s);
        launch_match(h->d_match_a, n, h->d_match_b, long(nb), lo, hi, ratio, splits, p_best, p_index, p_second,
                     d_match + at, best, second, n_over, s);
    }
    LF_HIP(h, hipGetLastError());
    return LF_MKD_OK;
}

int lf_mkd_match_device(lf_mkd *h, const float *d_a, uint64_t na, const float *d_b, uint64_t nb,
                        const uint32_t *d_exclude_lo, const uint32_t *d_exclude_hi, float ratio, int32_t *d_match,
                        float *d_best, float *d_second, void *stream) {
    return match_device_impl(h, d_a, na, d_b, nb, d_exclude_lo, d_exclude_hi, ratio, d_match, d_best, d_second, stream, false);
}

int lf_mkd_match_both_device(lf_mkd *h, const float *d_a, uint64_t na, const float *d_b, uint64_t nb, float ratio,
                             int32_t *d_match_ab, int32_t *d_match_ba, void *stream) {
    if (!h) return LF_MKD_ERR_BAD_ARG;
    // an empty side: nothing to match in either direction, nothing is written (as lf_mkd_match_device with na == 0)
    if (na == 0 || nb == 0) return LF_MKD_OK;
    if (!d_a || !d_b || !d_match_ab || !d_match_ba) return fail(h, LF_MKD_ERR_BAD_ARG, "match_both_device: null pointer");
    if (na < 2 || nb < 2) return fail(h, LF_MKD_ERR_BAD_ARG, "match_both: needs at least two rows on either side (main.rs:20)");
    if ((reinterpret_cast<uintptr_t>(d_a) | reinterpret_cast<uintptr_t>(d_b)) & 15)
        return fail(h, LF_MKD_ERR_BAD_ARG, "match_both_device: d_a and d_b must be 16-byte aligned");
    LF_ENTER(h);
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : h->stream;
    const char *form = getenv("LF_MKD_MATCH");
    if (!form && match_small_fits(long(na), long(nb)) && match_small_fits(long(nb), long(na))) {
        launch_match_small_both(d_a, long(na), d_b, long(nb), ratio, d_match_ab, d_match_ba,
                                h->d_match_misc ? h->d_match_misc + 2 : nullptr, s);
        LF_HIP(h, hipGetLastError());
        return LF_MKD_OK;
    }
    // larger problems (or a forced form): one call per direction, each in the form its size takes; the second adds its
    // redone rows to the first's, so that lf_mkd_match_overflowed reports on the whole call
    if (int rc = ensure_match_misc(h, s)) return rc;
    if (int rc = match_device_impl(h, d_a, na, d_b, nb, nullptr, nullptr, ratio, d_match_ab, nullptr, nullptr, s, false)) return rc;
    return match_device_impl(h, d_b, nb, d_a, na, nullptr, nullptr, ratio, d_match_ba, nullptr, nullptr, s, true);
}

// Many pairs in one call.  Like the verifiers it feeds, it checks its arguments before the handle, so that every bad
// argument is reported without a device: the message goes to the handle, or to lf_mkd_last_error(NULL) when there is none.
int lf_mkd_match_pairs_device(lf_mkd *h, const float *d_a, const uint64_t *d_offsets_a, uint64_t na_total, const float *d_b,
                              const uint64_t *d_offsets_b, uint64_t nb_total, uint32_t n_pairs, float ratio, uint32_t flags,
                              int32_t *d_match_ab, int32_t *d_match_ba, float *d_best, float *d_second, void *stream) {
    const bool mutual = flags & LF_MKD_MATCH_MUTUAL;
    const char *msg = nullptr;
    if (!d_a || !d_b || !d_offsets_a || !d_offsets_b || !d_match_ab) msg = "null pointer";
    else if (flags & ~LF_MKD_MATCH_MUTUAL) msg = "unknown flag bits";
    else if (mutual && !d_match_ba) msg = "LF_MKD_MATCH_MUTUAL needs d_match_ba";
    else if ((reinterpret_cast<uintptr_t>(d_a) | reinterpret_cast<uintptr_t>(d_b)) & 15) msg = "d_a and d_b must be 16-byte aligned";
    else if (na_total > 0x7FFFFFFFull || nb_total > 0x7FFFFFFFull) msg = "more than 2^31 - 1 rows on a side";
    else if (match_pairs_slots(na_total, n_pairs) + (d_match_ba ? match_pairs_slots(nb_total, n_pairs) : 0) > 0x7FFFFFFFull)
        msg = "too many rows and pairs for one call (the grid needs floor(rows / 16) + n_pairs workgroups per direction, "
              "at most 2^31 - 1 in all)";
    else if (!h) msg = "null handle";
    if (msg) {
        (h ? h->err : g_create_error) = std::string("match_pairs_device: ") + msg;
        return LF_MKD_ERR_BAD_ARG;
    }
    if (n_pairs == 0) return LF_MKD_OK;
    LF_ENTER(h);
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : h->stream;
    launch_match_small_pairs(d_a, d_offsets_a, na_total, d_b, d_offsets_b, nb_total, n_pairs, ratio, mutual, d_match_ab,
                             d_match_ba, d_best, d_second, h->d_match_misc ? h->d_match_misc + 2 : nullptr, s);
    LF_HIP(h, hipGetLastError());
    return LF_MKD_OK;
}

// Guided matching: the same batch under each pair's verified model.  Arguments are checked as above, before the handle.
int lf_mkd_match_guided_pairs_device(lf_mkd *h, const float *d_a, const lf_mkd_keypoint *d_kps_a, const uint64_t *d_offsets_a,
                                     uint64_t na_total, const float *d_b, const lf_mkd_keypoint *d_kps_b,
                                     const uint64_t *d_offsets_b, uint64_t nb_total, const float *d_model, uint32_t n_pairs,
                                     uint32_t kind, float threshold_px, float ratio, uint32_t flags, int32_t *d_match_ab,
                                     int32_t *d_match_ba, float *d_best, float *d_second, void *stream) {
    const bool mutual = flags & LF_MKD_MATCH_MUTUAL;
    const char *msg = nullptr;
    if (!d_a || !d_b || !d_kps_a || !d_kps_b || !d_offsets_a || !d_offsets_b || !d_model || !d_match_ab) msg = "null pointer";
    else if (flags & ~LF_MKD_MATCH_MUTUAL) msg = "unknown flag bits";
    else if (mutual && !d_match_ba) msg = "LF_MKD_MATCH_MUTUAL needs d_match_ba";
    else if (kind > LF_MKD_GUIDE_FUNDAMENTAL) msg = "kind must be LF_MKD_GUIDE_HOMOGRAPHY or LF_MKD_GUIDE_FUNDAMENTAL";
    // (the verifiers' rule, verify_args below: the kernel compares against thr^2 in f32)
    else if (!(threshold_px > 0.f) || !std::isnormal(threshold_px * threshold_px))
        msg = "threshold_px must be positive, with a finite normal f32 square (about 1.09e-19 .. 1.84e19)";
    else if ((reinterpret_cast<uintptr_t>(d_a) | reinterpret_cast<uintptr_t>(d_b)) & 15) msg = "d_a and d_b must be 16-byte aligned";
    else if (na_total > 0x7FFFFFFFull || nb_total > 0x7FFFFFFFull) msg = "more than 2^31 - 1 rows on a side";
    else if (match_pairs_slots(na_total, n_pairs) + (d_match_ba ? match_pairs_slots(nb_total, n_pairs) : 0) > 0x7FFFFFFFull)
        msg = "too many rows and pairs for one call (the grid needs floor(rows / 16) + n_pairs workgroups per direction, "
              "at most 2^31 - 1 in all)";
    else if (!h) msg = "null handle";
    if (msg) {
        (h ? h->err : g_create_error) = std::string("match_guided_pairs_device: ") + msg;
        return LF_MKD_ERR_BAD_ARG;
    }
    if (n_pairs == 0) return LF_MKD_OK;
    LF_ENTER(h);
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : h->stream;
    launch_match_guided_pairs(d_a, reinterpret_cast<const float *>(d_kps_a), d_offsets_a, na_total, d_b,
                              reinterpret_cast<const float *>(d_kps_b), d_offsets_b, nb_total, d_model, n_pairs, kind,
                              threshold_px, ratio, mutual, d_match_ab, d_match_ba, d_best, d_second, s);
    LF_HIP(h, hipGetLastError());
    return LF_MKD_OK;
}

int lf_mkd_match_overflowed(lf_mkd *h, void *stream, uint64_t *n_rows) {
    if (!h) return LF_MKD_ERR_BAD_ARG;
    if (!n_rows) return fail(h, LF_MKD_ERR_BAD_ARG, "match_overflowed: null pointer");
    *n_rows = 0;
    if (!h->d_match_misc) return LF_MKD_OK;           // no two-pass match yet
    LF_ENTER(h);
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : h->stream;
    int n = 0;
    LF_HIP(h, hipMemcpyAsync(&n, h->d_match_misc + 2, sizeof(int), hipMemcpyDeviceToHost, s));
    LF_HIP(h, hipStreamSynchronize(s));
    *n_rows = uint64_t(n);
    return LF_MKD_OK;
}

int lf_mkd_match(lf_mkd *h, const float *a, uint64_t na, const float *b, uint64_t nb, float ratio, int32_t *match) {
    if (!h) return LF_MKD_ERR_BAD_ARG;
    if (na == 0) return LF_MKD_OK;
    if (!a || !b || !match) return fail(h, LF_MKD_ERR_BAD_ARG, "match: null pointer");
    if (nb < 2) return fail(h, LF_MKD_ERR_BAD_ARG, "match: needs at least two candidates in b (main.rs:20)");
    LF_ENTER(h);
    if (int rc = grow(h, h->d_match_in, (na + nb) * kOut)) return rc;
    if (int rc = grow(h, h->d_match_out, na)) return rc;
    LF_HIP(h, hipMemcpyAsync(h->d_match_in, a, na * kOut * 4, hipMemcpyHostToDevice, h->stream));
    LF_HIP(h, hipMemcpyAsync(h->d_match_in + na * kOut, b, nb * kOut * 4, hipMemcpyHostToDevice, h->stream));
    if (int rc = lf_mkd_match_device(h, h->d_match_in, na, h->d_match_in + na * kOut, nb, nullptr, nullptr, ratio,
                                     h->d_match_out, nullptr, nullptr, h->stream))
        return rc;
    LF_HIP(h, hipMemcpyAsync(match, h->d_match_out, na * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    LF_HIP(h, hipStreamSynchronize(h->stream));
    return LF_MKD_OK;
}

// ---- 8-bit descriptors (csrc/mkd_match_q8.hip) --------------------------------------------------------------------------
// Like the batched calls above, these check their arguments before the handle, so that every bad argument is reported
// without a device: the message goes to the handle, or to lf_mkd_last_error(NULL) when there is none.
static int q8_refuse(lf_mkd *h, const char *who, const char *msg) {
    (h ? h->err : g_create_error) = std::string(who) + ": " + msg;
    return LF_MKD_ERR_BAD_ARG;
}

// 0 -> the default; nullptr: fine
static const char *q8_scale(float &scale) {
    if (scale == 0.f) scale = 256.f;
    return scale > 0.f && std::isnormal(scale) ? nullptr : "scale must be a positive, finite, normal f32 (0: the default, 256)";
}

static const char *quantize_args(const lf_mkd *h, const void *desc, uint64_t n, float &scale, const void *q, bool device) {
    if (const char *msg = q8_scale(scale)) return msg;
    if (n && (!desc || !q)) return "null pointer";
    if (n > 0x7FFFFFFFull) return "more than 2^31 - 1 rows";
    if (device && n && ((reinterpret_cast<uintptr_t>(desc) & 15) || (reinterpret_cast<uintptr_t>(q) & 3)))
        return "d_desc must be 16-byte aligned and d_q 4-byte aligned";
    return h ? nullptr : "null handle";
}

int lf_mkd_quantize_descriptors_device(lf_mkd *h, const float *d_desc, uint64_t n, float scale, uint8_t *d_q, void *stream) {
    if (const char *msg = quantize_args(h, d_desc, n, scale, d_q, true)) return q8_refuse(h, "quantize_descriptors_device", msg);
    if (n == 0) return LF_MKD_OK;
    LF_ENTER(h);
    launch_quantize_rows(d_desc, n, scale, d_q, stream ? static_cast<hipStream_t>(stream) : h->stream);
    LF_HIP(h, hipGetLastError());
    return LF_MKD_OK;
}

int lf_mkd_quantize_descriptors(lf_mkd *h, const float *desc, uint64_t n, float scale, uint8_t *q) {
    if (const char *msg = quantize_args(h, desc, n, scale, q, false)) return q8_refuse(h, "quantize_descriptors", msg);
    if (n == 0) return LF_MKD_OK;
    LF_ENTER(h);
    if (int rc = grow(h, h->d_match_in, n * kOut)) return rc;
    if (int rc = grow(h, h->d_q8_io, n * kOut)) return rc;
    LF_HIP(h, hipMemcpyAsync(h->d_match_in, desc, n * kOut * sizeof(float), hipMemcpyHostToDevice, h->stream));
    launch_quantize_rows(h->d_match_in, n, scale, h->d_q8_io, h->stream);
    LF_HIP(h, hipGetLastError());
    LF_HIP(h, hipMemcpyAsync(q, h->d_q8_io, n * kOut, hipMemcpyDeviceToHost, h->stream));
    LF_HIP(h, hipStreamSynchronize(h->stream));
    return LF_MKD_OK;
}

static const char *match_q8_sizes(uint64_t na, uint64_t nb) {
    if (nb < 2) return "needs at least two candidates in b";
    if (na > 0x7FFFFFFFull || nb > 0x7FFFFFFFull) return "more than 2^31 - 1 rows on a side";
    return nullptr;
}

int lf_mkd_match_q8_plan(uint64_t na, uint64_t nb, uint32_t num_cus, uint32_t *a_blocks, uint32_t *b_splits,
                         uint64_t *scratch_bytes) {
    if (const char *msg = match_q8_sizes(na, nb)) return q8_refuse(nullptr, "match_q8_plan", msg);
    const Q8Plan p = match_q8_plan(long(na), long(nb), int(std::min<uint32_t>(num_cus, 1u << 20)));
    if (a_blocks) *a_blocks = p.a_blocks;
    if (b_splits) *b_splits = p.splits;
    if (scratch_bytes) *scratch_bytes = p.scratch_bytes;
    return LF_MKD_OK;
}

static const char *match_q8_args(const lf_mkd *h, const void *a, uint64_t na, const void *b, uint64_t nb, const void *lo,
                                 const void *hi, const void *match, bool device) {
    if (na && (!a || !b || !match)) return "null pointer";
    if ((lo == nullptr) != (hi == nullptr)) return "exclude_lo and exclude_hi go together";
    if (device && na && ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 15))
        return "d_a and d_b must be 16-byte aligned";
    if (const char *msg = match_q8_sizes(na, nb)) return msg;
    return h ? nullptr : "null handle";
}

int lf_mkd_match_q8_device(lf_mkd *h, const uint8_t *d_a, uint64_t na, const uint8_t *d_b, uint64_t nb,
                           const uint32_t *d_exclude_lo, const uint32_t *d_exclude_hi, float ratio, int32_t *d_match,
                           int32_t *d_best, int32_t *d_second, void *stream) {
    if (const char *msg = match_q8_args(h, d_a, na, d_b, nb, d_exclude_lo, d_exclude_hi, d_match, true))
        return q8_refuse(h, "match_q8_device", msg);
    if (na == 0) return LF_MKD_OK;
    LF_ENTER(h);
    const Q8Plan plan = match_q8_plan(long(na), long(nb), h->num_cus);
    if (plan.scratch_bytes)
        if (int rc = grow(h, h->d_q8_part, plan.scratch_bytes)) return rc;
    launch_match_q8(d_a, long(na), d_b, long(nb), d_exclude_lo, d_exclude_hi, ratio, plan,
                    plan.scratch_bytes ? h->d_q8_part.get() : nullptr, d_match, d_best, d_second,
                    stream ? static_cast<hipStream_t>(stream) : h->stream);
    LF_HIP(h, hipGetLastError());
    return LF_MKD_OK;
}

int lf_mkd_match_q8(lf_mkd *h, const uint8_t *a, uint64_t na, const uint8_t *b, uint64_t nb, float ratio, int32_t *match) {
    if (const char *msg = match_q8_args(h, a, na, b, nb, nullptr, nullptr, match, false)) return q8_refuse(h, "match_q8", msg);
    if (na == 0) return LF_MKD_OK;
    LF_ENTER(h);
    if (int rc = grow(h, h->d_q8_io, (na + nb) * kOut)) return rc;
    if (int rc = grow(h, h->d_match_out, na)) return rc;
    LF_HIP(h, hipMemcpyAsync(h->d_q8_io, a, na * kOut, hipMemcpyHostToDevice, h->stream));
    LF_HIP(h, hipMemcpyAsync(h->d_q8_io + na * kOut, b, nb * kOut, hipMemcpyHostToDevice, h->stream));
    if (int rc = lf_mkd_match_q8_device(h, h->d_q8_io, na, h->d_q8_io + na * kOut, nb, nullptr, nullptr, ratio, h->d_match_out,
                                        nullptr, nullptr, h->stream))
        return rc;
    LF_HIP(h, hipMemcpyAsync(match, h->d_match_out, na * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    LF_HIP(h, hipStreamSynchronize(h->stream));
    return LF_MKD_OK;
}

// The exact top-k over 8-bit rows (csrc/mkd_match_q8_knn.hip): the matcher's refusals, except that one candidate is an answer.
static const char *knn_q8_sizes(uint64_t na, uint64_t nb, uint32_t k) {
    if (k == 0 || k > LF_MKD_KNN_MAX) return "k must be 1 .. LF_MKD_KNN_MAX (16)";
    if (nb == 0) return "needs at least one candidate in b";
    if (na > 0x7FFFFFFFull || nb > 0x7FFFFFFFull) return "more than 2^31 - 1 rows on a side";
    return nullptr;
}

int lf_mkd_knn_q8_plan(uint64_t na, uint64_t nb, uint32_t k, uint32_t num_cus, uint32_t *a_blocks, uint32_t *b_splits,
                       uint64_t *scratch_bytes) {
    if (const char *msg = knn_q8_sizes(na, nb, k)) return q8_refuse(nullptr, "knn_q8_plan", msg);
    const KnnQ8Plan p = knn_q8_plan(long(na), long(nb), int(k), int(std::min<uint32_t>(num_cus, 1u << 20)));
    if (a_blocks) *a_blocks = p.a_blocks;
    if (b_splits) *b_splits = p.splits;
    if (scratch_bytes) *scratch_bytes = p.scratch_bytes;
    return LF_MKD_OK;
}

static const char *knn_q8_args(const lf_mkd *h, const void *a, uint64_t na, const void *b, uint64_t nb, const void *lo,
                               const void *hi, uint32_t k, const void *index, bool device) {
    if (na && (!a || !b || !index)) return "null pointer";
    if ((lo == nullptr) != (hi == nullptr)) return "exclude_lo and exclude_hi go together";
    if (device && na && ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 15))
        return "d_a and d_b must be 16-byte aligned";
    if (const char *msg = knn_q8_sizes(na, nb, k)) return msg;
    return h ? nullptr : "null handle";
}

int lf_mkd_knn_q8_device(lf_mkd *h, const uint8_t *d_a, uint64_t na, const uint8_t *d_b, uint64_t nb,
                         const uint32_t *d_exclude_lo, const uint32_t *d_exclude_hi, uint32_t k, int32_t *d_index,
                         int32_t *d_score, void *stream) {
    if (const char *msg = knn_q8_args(h, d_a, na, d_b, nb, d_exclude_lo, d_exclude_hi, k, d_index, true))
        return q8_refuse(h, "knn_q8_device", msg);
    if (na == 0) return LF_MKD_OK;
    LF_ENTER(h);
    const KnnQ8Plan plan = knn_q8_plan(long(na), long(nb), int(k), h->num_cus);
    if (plan.scratch_bytes)
        if (int rc = grow(h, h->d_q8_part, plan.scratch_bytes)) return rc;
    launch_knn_q8(d_a, long(na), d_b, long(nb), d_exclude_lo, d_exclude_hi, int(k), plan,
                  plan.scratch_bytes ? h->d_q8_part.get() : nullptr, d_index, d_score,
                  stream ? static_cast<hipStream_t>(stream) : h->stream);
    LF_HIP(h, hipGetLastError());
    return LF_MKD_OK;
}

int lf_mkd_knn_q8(lf_mkd *h, const uint8_t *a, uint64_t na, const uint8_t *b, uint64_t nb, uint32_t k, int32_t *index,
                  int32_t *score) {
    if (const char *msg = knn_q8_args(h, a, na, b, nb, nullptr, nullptr, k, index, false)) return q8_refuse(h, "knn_q8", msg);
    if (na == 0) return LF_MKD_OK;
    LF_ENTER(h);
    if (int rc = grow(h, h->d_q8_io, (na + nb) * kOut)) return rc;
    if (int rc = grow(h, h->d_match_out, 2 * na * k)) return rc;
    LF_HIP(h, hipMemcpyAsync(h->d_q8_io, a, na * kOut, hipMemcpyHostToDevice, h->stream));
    LF_HIP(h, hipMemcpyAsync(h->d_q8_io + na * kOut, b, nb * kOut, hipMemcpyHostToDevice, h->stream));
    if (int rc = lf_mkd_knn_q8_device(h, h->d_q8_io, na, h->d_q8_io + na * kOut, nb, nullptr, nullptr, k, h->d_match_out,
                                      score ? h->d_match_out + na * k : nullptr, h->stream))
        return rc;
    LF_HIP(h, hipMemcpyAsync(index, h->d_match_out, na * k * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    if (score) LF_HIP(h, hipMemcpyAsync(score, h->d_match_out + na * k, na * k * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    LF_HIP(h, hipStreamSynchronize(h->stream));
    return LF_MKD_OK;
}

// Grouped matching over 8-bit rows (csrc/mkd_match_q8_grouped.hip): the matcher's refusals, except that one candidate is an
// answer; the rival is the best score of another group than the best's.
static const char *match_q8_grouped_sizes(uint64_t na, uint64_t nb) {
    if (nb == 0) return "needs at least one candidate in b";
    if (na > 0x7FFFFFFFull || nb > 0x7FFFFFFFull) return "more than 2^31 - 1 rows on a side";
    return nullptr;
}

int lf_mkd_match_q8_grouped_plan(uint64_t na, uint64_t nb, uint32_t num_cus, uint32_t *a_blocks, uint32_t *b_splits,
                                 uint64_t *scratch_bytes) {
    if (const char *msg = match_q8_grouped_sizes(na, nb)) return q8_refuse(nullptr, "match_q8_grouped_plan", msg);
    const Q8GroupedPlan p = match_q8_grouped_plan(long(na), long(nb), int(std::min<uint32_t>(num_cus, 1u << 20)));
    if (a_blocks) *a_blocks = p.a_blocks;
    if (b_splits) *b_splits = p.splits;
    if (scratch_bytes) *scratch_bytes = p.scratch_bytes;
    return LF_MKD_OK;
}

static const char *match_q8_grouped_args(const lf_mkd *h, const void *a, uint64_t na, const void *b, uint64_t nb,
                                         const void *group, const void *lo, const void *hi, const void *match,
                                         const void *best, const void *rival, bool device) {
    if (na && (!a || !b || !group || !match)) return "null pointer";
    if ((lo == nullptr) != (hi == nullptr)) return "exclude_lo and exclude_hi go together";
    if (device && na && ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 15))
        return "d_a and d_b must be 16-byte aligned";
    if (device && na && ((reinterpret_cast<uintptr_t>(group) | reinterpret_cast<uintptr_t>(lo) | reinterpret_cast<uintptr_t>(hi) |
                          reinterpret_cast<uintptr_t>(match) | reinterpret_cast<uintptr_t>(best) |
                          reinterpret_cast<uintptr_t>(rival)) & 3))
        return "d_group_of_b, the exclusion bounds and the outputs must be 4-byte aligned";
    if (const char *msg = match_q8_grouped_sizes(na, nb)) return msg;
    return h ? nullptr : "null handle";
}

int lf_mkd_match_q8_grouped_device(lf_mkd *h, const uint8_t *d_a, uint64_t na, const uint8_t *d_b, uint64_t nb,
                                   const uint32_t *d_group_of_b, const uint32_t *d_exclude_lo, const uint32_t *d_exclude_hi,
                                   float ratio, int32_t *d_match, int32_t *d_best, int32_t *d_rival, void *stream) {
    if (const char *msg = match_q8_grouped_args(h, d_a, na, d_b, nb, d_group_of_b, d_exclude_lo, d_exclude_hi, d_match, d_best,
                                                d_rival, true))
        return q8_refuse(h, "match_q8_grouped_device", msg);
    if (na == 0) return LF_MKD_OK;
    LF_ENTER(h);
    const Q8GroupedPlan plan = match_q8_grouped_plan(long(na), long(nb), h->num_cus);
    if (plan.scratch_bytes)
        if (int rc = grow(h, h->d_q8_part, plan.scratch_bytes)) return rc;
    launch_match_q8_grouped(d_a, long(na), d_b, long(nb), d_group_of_b, d_exclude_lo, d_exclude_hi, ratio, plan,
                            plan.scratch_bytes ? h->d_q8_part.get() : nullptr, d_match, d_best, d_rival,
                            stream ? static_cast<hipStream_t>(stream) : h->stream);
    LF_HIP(h, hipGetLastError());
    return LF_MKD_OK;
}

int lf_mkd_match_q8_grouped(lf_mkd *h, const uint8_t *a, uint64_t na, const uint8_t *b, uint64_t nb,
                            const uint32_t *group_of_b, float ratio, int32_t *match, int32_t *best, int32_t *rival) {
    if (const char *msg = match_q8_grouped_args(h, a, na, b, nb, group_of_b, nullptr, nullptr, match, best, rival, false))
        return q8_refuse(h, "match_q8_grouped", msg);
    if (na == 0) return LF_MKD_OK;
    LF_ENTER(h);
    // the staging holds a's rows, b's rows and then b's group ids ((na + nb) * 128 keeps them 4-byte aligned)
    if (int rc = grow(h, h->d_q8_io, (na + nb) * kOut + nb * sizeof(uint32_t))) return rc;
    if (int rc = grow(h, h->d_match_out, 3 * na)) return rc;
    unsigned char *d_b = h->d_q8_io + na * kOut;
    uint32_t *d_group = reinterpret_cast<uint32_t *>(h->d_q8_io + (na + nb) * kOut);
    LF_HIP(h, hipMemcpyAsync(h->d_q8_io, a, na * kOut, hipMemcpyHostToDevice, h->stream));
    LF_HIP(h, hipMemcpyAsync(d_b, b, nb * kOut, hipMemcpyHostToDevice, h->stream));
    LF_HIP(h, hipMemcpyAsync(d_group, group_of_b, nb * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
    if (int rc = lf_mkd_match_q8_grouped_device(h, h->d_q8_io, na, d_b, nb, d_group, nullptr, nullptr, ratio, h->d_match_out,
                                                best ? h->d_match_out + na : nullptr,
                                                rival ? h->d_match_out + 2 * na : nullptr, h->stream))
        return rc;
    LF_HIP(h, hipMemcpyAsync(match, h->d_match_out, na * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    if (best) LF_HIP(h, hipMemcpyAsync(best, h->d_match_out + na, na * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    if (rival) LF_HIP(h, hipMemcpyAsync(rival, h->d_match_out + 2 * na, na * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    LF_HIP(h, hipStreamSynchronize(h->stream));
    return LF_MKD_OK;
}

// The group-by-group vote table of a match array: a zeroing launch and one launch of integer atomic adds.
int lf_mkd_vote_groups_device(lf_mkd *h, const int32_t *d_match, uint64_t na, const uint32_t *d_group_of_a, uint32_t n_groups_a,
                              const uint32_t *d_group_of_b, uint64_t nb, uint32_t n_groups_b, uint32_t *d_votes, void *stream) {
    const char *msg = nullptr;
    if (na && (!d_match || !d_group_of_b)) msg = "null pointer";
    else if (n_groups_a == 0 || n_groups_b == 0) msg = "a group count of zero";
    else if (uint64_t(n_groups_a) * n_groups_b > 0x7FFFFFFFull) msg = "more than 2^31 - 1 entries in the vote table";
    else if (!d_votes) msg = "null d_votes";
    else if (na > 0x7FFFFFFFull || nb > 0x7FFFFFFFull) msg = "more than 2^31 - 1 rows on a side";
    else if ((reinterpret_cast<uintptr_t>(d_match) | reinterpret_cast<uintptr_t>(d_group_of_a) |
              reinterpret_cast<uintptr_t>(d_group_of_b) | reinterpret_cast<uintptr_t>(d_votes)) & 3)
        msg = "the arrays must be 4-byte aligned";
    else if (!h) msg = "null handle";
    if (msg) return q8_refuse(h, "vote_groups_device", msg);
    LF_ENTER(h);
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : h->stream;
    launch_vote_groups(d_match, long(na), d_group_of_a, n_groups_a, d_group_of_b, long(nb), n_groups_b, d_votes, s);
    LF_HIP(h, hipGetLastError());
    return LF_MKD_OK;
}

// Many pairs of 8-bit rows in one call: lf_mkd_match_pairs_device's layout and refusals, the int8 matcher's decisions.
static const char *match_q8_pairs_sizes(uint64_t na_total, uint64_t nb_total, uint32_t n_pairs, bool both) {
    if (na_total > 0x7FFFFFFFull || nb_total > 0x7FFFFFFFull) return "more than 2^31 - 1 rows on a side";
    if (match_q8_pairs_slots(na_total, n_pairs) + (both ? match_q8_pairs_slots(nb_total, n_pairs) : 0) > 0x7FFFFFFFull)
        return "too many rows and pairs for one call (the grid needs floor(rows / block_rows) + n_pairs workgroups per "
               "direction, at most 2^31 - 1 in all)";
    return nullptr;
}

int lf_mkd_match_q8_pairs_plan(uint64_t na_total, uint64_t nb_total, uint32_t n_pairs, uint32_t both_directions,
                               uint32_t *block_rows, uint64_t *workgroups) {
    if (const char *msg = match_q8_pairs_sizes(na_total, nb_total, n_pairs, both_directions != 0))
        return q8_refuse(nullptr, "match_q8_pairs_plan", msg);
    if (block_rows) *block_rows = match_q8_pairs_block_rows();
    if (workgroups)
        *workgroups = match_q8_pairs_slots(na_total, n_pairs) + (both_directions ? match_q8_pairs_slots(nb_total, n_pairs) : 0);
    return LF_MKD_OK;
}

int lf_mkd_match_q8_pairs_device(lf_mkd *h, const uint8_t *d_a, const uint64_t *d_offsets_a, uint64_t na_total,
                                 const uint8_t *d_b, const uint64_t *d_offsets_b, uint64_t nb_total, uint32_t n_pairs,
                                 float ratio, uint32_t flags, int32_t *d_match_ab, int32_t *d_match_ba, int32_t *d_best,
                                 int32_t *d_second, void *stream) {
    const bool mutual = flags & LF_MKD_MATCH_MUTUAL;
    const char *msg = nullptr;
    if (!d_a || !d_b || !d_offsets_a || !d_offsets_b || !d_match_ab) msg = "null pointer";
    else if (flags & ~LF_MKD_MATCH_MUTUAL) msg = "unknown flag bits";
    else if (mutual && !d_match_ba) msg = "LF_MKD_MATCH_MUTUAL needs d_match_ba";
    else if ((reinterpret_cast<uintptr_t>(d_a) | reinterpret_cast<uintptr_t>(d_b)) & 15) msg = "d_a and d_b must be 16-byte aligned";
    else if (!(msg = match_q8_pairs_sizes(na_total, nb_total, n_pairs, d_match_ba != nullptr)) && !h) msg = "null handle";
    if (msg) return q8_refuse(h, "match_q8_pairs_device", msg);
    if (n_pairs == 0) return LF_MKD_OK;
    LF_ENTER(h);
    launch_match_q8_pairs(d_a, d_offsets_a, na_total, d_b, d_offsets_b, nb_total, n_pairs, ratio, mutual, d_match_ab, d_match_ba,
                          d_best, d_second, stream ? static_cast<hipStream_t>(stream) : h->stream);
    LF_HIP(h, hipGetLastError());
    return LF_MKD_OK;
}

// Edge-list matching over 8-bit rows (csrc/mkd_match_q8_edges.hip): pools, edges and edge layouts.  Every refusal comes
// before the handle is looked at, so it is reported without a device.
static const uint64_t kEdgeMax = 0x7FFFFFFFull;

int lf_mkd_edge_layout_device(lf_mkd *h, const uint64_t *d_image_offsets, uint32_t n_images, uint64_t n_rows_total,
                              const uint32_t *d_edge_image, uint32_t n_edges, uint64_t *d_edge_offsets, void *stream) {
    const char *msg = nullptr;
    if (n_edges && (!d_image_offsets || !d_edge_image || !d_edge_offsets)) msg = "null pointer";
    else if ((reinterpret_cast<uintptr_t>(d_image_offsets) | reinterpret_cast<uintptr_t>(d_edge_offsets)) & 7)
        msg = "the offset arrays must be 8-byte aligned";
    else if (reinterpret_cast<uintptr_t>(d_edge_image) & 3) msg = "d_edge_image must be 4-byte aligned";
    else if (n_rows_total > kEdgeMax) msg = "more than 2^31 - 1 rows in the pool";
    else if (!h) msg = "null handle";
    if (msg) return q8_refuse(h, "edge_layout_device", msg);
    if (n_edges == 0) return LF_MKD_OK;
    LF_ENTER(h);
    launch_edge_layout(d_image_offsets, n_images, n_rows_total, d_edge_image, n_edges, d_edge_offsets,
                       stream ? static_cast<hipStream_t>(stream) : h->stream);
    LF_HIP(h, hipGetLastError());
    return LF_MKD_OK;
}

int lf_mkd_gather_edge_rows_device(lf_mkd *h, const void *d_src, uint32_t row_bytes, const uint64_t *d_image_offsets,
                                   uint32_t n_images, uint64_t n_rows_total, const uint32_t *d_edge_image,
                                   const uint64_t *d_edge_offsets, uint64_t capacity_rows, uint32_t n_edges, void *d_dst,
                                   void *stream) {
    const char *msg = nullptr;
    if (!d_src || !d_image_offsets || !d_edge_image || !d_edge_offsets || !d_dst) msg = "null pointer";
    else if (row_bytes < 4 || row_bytes > 512 || (row_bytes & 3)) msg = "row_bytes must be a multiple of 4 in [4, 512]";
    else if ((reinterpret_cast<uintptr_t>(d_src) | reinterpret_cast<uintptr_t>(d_dst)) & 3) msg = "d_src and d_dst must be 4-byte aligned";
    else if (n_rows_total > kEdgeMax || capacity_rows > kEdgeMax) msg = "a total or a capacity above 2^31 - 1 rows";
    else if (capacity_rows / gather_edge_rows_block_rows() + n_edges > kEdgeMax)
        msg = "too many rows and edges for one call (the grid needs floor(capacity / block_rows) + n_edges workgroups, at most 2^31 - 1)";
    else if (!h) msg = "null handle";
    if (msg) return q8_refuse(h, "gather_edge_rows_device", msg);
    if (n_edges == 0) return LF_MKD_OK;
    LF_ENTER(h);
    launch_gather_edge_rows(d_src, row_bytes, d_image_offsets, n_images, n_rows_total, d_edge_image, d_edge_offsets, capacity_rows,
                            n_edges, d_dst, stream ? static_cast<hipStream_t>(stream) : h->stream);
    LF_HIP(h, hipGetLastError());
    return LF_MKD_OK;
}

int lf_mkd_match_q8_edges_device(lf_mkd *h, const uint8_t *d_a, const uint64_t *d_image_offsets_a, uint32_t n_images_a,
                                 uint64_t na_total, const uint8_t *d_b, const uint64_t *d_image_offsets_b, uint32_t n_images_b,
                                 uint64_t nb_total, const uint32_t *d_edge_a, const uint32_t *d_edge_b,
                                 const uint64_t *d_edge_offsets_a, uint64_t ea_capacity, const uint64_t *d_edge_offsets_b,
                                 uint64_t eb_capacity, uint32_t n_edges, float ratio, uint32_t flags, int32_t *d_match_ab,
                                 int32_t *d_match_ba, int32_t *d_best, int32_t *d_second, void *stream) {
    const bool mutual = flags & LF_MKD_MATCH_MUTUAL;
    const char *msg = nullptr;
    if (!d_a || !d_b || !d_image_offsets_a || !d_image_offsets_b || !d_match_ab) msg = "null pointer";
    else if (!d_edge_a || !d_edge_b) msg = "null edge array";
    else if (!d_edge_offsets_a) msg = "null layout array";
    else if (flags & ~LF_MKD_MATCH_MUTUAL) msg = "unknown flag bits";
    else if (mutual && !d_match_ba) msg = "LF_MKD_MATCH_MUTUAL needs d_match_ba";
    else if (d_match_ba && !d_edge_offsets_b) msg = "null layout array: d_match_ba needs d_edge_offsets_b";
    else if ((reinterpret_cast<uintptr_t>(d_a) | reinterpret_cast<uintptr_t>(d_b)) & 15) msg = "d_a and d_b must be 16-byte aligned";
    else if (na_total > kEdgeMax || nb_total > kEdgeMax || ea_capacity > kEdgeMax || eb_capacity > kEdgeMax)
        msg = "a total or a capacity above 2^31 - 1 rows";
    // the grid is the pairs call's over the capacities: the same plan, the same words
    else if (!(msg = match_q8_pairs_sizes(ea_capacity, eb_capacity, n_edges, d_match_ba != nullptr)) && !h) msg = "null handle";
    if (msg) return q8_refuse(h, "match_q8_edges_device", msg);
    if (n_edges == 0) return LF_MKD_OK;
    LF_ENTER(h);
    launch_match_q8_edges(d_a, d_image_offsets_a, n_images_a, na_total, d_b, d_image_offsets_b, n_images_b, nb_total, d_edge_a,
                          d_edge_b, d_edge_offsets_a, ea_capacity, d_edge_offsets_b, eb_capacity, n_edges, ratio, mutual,
                          d_match_ab, d_match_ba, d_best, d_second, stream ? static_cast<hipStream_t>(stream) : h->stream);
    LF_HIP(h, hipGetLastError());
    return LF_MKD_OK;
}

// Feature tracks over an edge list's matches (csrc/mkd_tracks.hip).  The grids are sized here, from the arguments alone.
int lf_mkd_build_tracks_device(lf_mkd *h, const uint64_t *d_image_offsets, uint32_t n_images, uint64_t n_rows_total,
                               const uint32_t *d_edge_a, const uint32_t *d_edge_b, const uint64_t *d_edge_offsets_a,
                               uint64_t ea_capacity, uint32_t n_edges, const int32_t *d_match, uint32_t flags,
                               int32_t *d_track, uint32_t *d_track_len, uint32_t *d_track_dup, void *stream) {
    const auto at = [](const void *p) { return reinterpret_cast<uintptr_t>(p); };
    const char *msg = nullptr;
    if (!d_image_offsets || !d_track) msg = "null pointer";
    else if (n_edges && (!d_edge_a || !d_edge_b)) msg = "null edge array";
    else if (n_edges && !d_edge_offsets_a) msg = "null layout array";
    else if (n_edges && !d_match) msg = "null match array";
    else if ((at(d_image_offsets) | at(d_edge_offsets_a)) & 7) msg = "the offset arrays must be 8-byte aligned";
    else if ((at(d_edge_a) | at(d_edge_b) | at(d_match) | at(d_track) | at(d_track_len) | at(d_track_dup)) & 3)
        msg = "the edge, match, track and statistics arrays must be 4-byte aligned";
    else if (flags & ~LF_MKD_TRACKS_ACCUMULATE) msg = "unknown flag bits";
    else if (n_rows_total > kEdgeMax || ea_capacity > kEdgeMax) msg = "a total or a capacity above 2^31 - 1 rows";
    else if (ea_capacity / build_tracks_link_entries() + n_edges > kEdgeMax)
        msg = "too many entries and edges for one call (the link grid needs floor(ea_capacity / 256) + n_edges workgroups, at "
              "most 2^31 - 1)";
    else if (d_track_dup && n_rows_total / build_tracks_dup_tile() + n_images > kEdgeMax)
        msg = "too many rows and images for one call (d_track_dup's grid needs floor(n_rows_total / LF_MKD_TRACKS_DUP_TILE) + "
              "n_images workgroups, at most 2^31 - 1)";
    else if (!h) msg = "null handle";
    if (msg) return q8_refuse(h, "build_tracks_device", msg);
    if (n_rows_total == 0) return LF_MKD_OK;
    LF_ENTER(h);
    launch_build_tracks(d_image_offsets, n_images, n_rows_total, d_edge_a, d_edge_b, d_edge_offsets_a, ea_capacity, n_edges,
                        d_match, (flags & LF_MKD_TRACKS_ACCUMULATE) != 0, d_track, d_track_len, d_track_dup,
                        stream ? static_cast<hipStream_t>(stream) : h->stream);
    LF_HIP(h, hipGetLastError());
    return LF_MKD_OK;
}

// Track tables (csrc/mkd_track_table.hip).  Every refusal comes before the handle is looked at.
int lf_mkd_track_table_plan(uint64_t n_rows_total, uint32_t min_len, uint32_t *key_bits, uint32_t *passes, uint32_t *block_rows,
                            uint64_t *scratch_bytes) {
    if (min_len == 0) return q8_refuse(nullptr, "track_table_plan", "min_len must be at least 1");
    if (n_rows_total > kEdgeMax) return q8_refuse(nullptr, "track_table_plan", "more than 2^31 - 1 rows in the pool");
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
    const auto at = [](const void *p) { return reinterpret_cast<uintptr_t>(p); };
    const bool consistent = flags & LF_MKD_TRACK_TABLE_CONSISTENT;
    const char *msg = nullptr;
    if (!d_track_offsets || !d_counts) msg = "null pointer";
    else if (n_rows_total && (!d_track || !d_track_len)) msg = "null track or length array";
    else if (obs_capacity && !d_obs_row) msg = "null d_obs_row";
    else if (d_obs_image && !d_image_offsets) msg = "d_obs_image needs d_image_offsets";
    else if (min_len == 0) msg = "min_len must be at least 1";
    else if (flags & ~LF_MKD_TRACK_TABLE_CONSISTENT) msg = "unknown flag bits";
    else if (consistent && n_rows_total && !d_track_dup) msg = "LF_MKD_TRACK_TABLE_CONSISTENT needs d_track_dup";
    else if ((at(d_image_offsets) | at(d_track_offsets)) & 7) msg = "the offset arrays must be 8-byte aligned";
    else if ((at(d_track) | at(d_track_len) | at(d_track_dup) | at(d_obs_row) | at(d_obs_image) | at(d_row_track) | at(d_counts)) & 3)
        msg = "the track, statistics, observation and count arrays must be 4-byte aligned";
    else if (n_rows_total > kEdgeMax || track_capacity > kEdgeMax || obs_capacity > kEdgeMax)
        msg = "a total or a capacity above 2^31 - 1";
    else if (!h) msg = "null handle";
    if (msg) return q8_refuse(h, "track_table_device", msg);
    LF_ENTER(h);
    const TrackTablePlan plan = track_table_plan(n_rows_total, min_len);
    if (plan.scratch_bytes)
        if (int rc = grow(h, h->d_track_table, plan.scratch_bytes)) return rc;
    launch_track_table(plan, plan.scratch_bytes ? h->d_track_table.get() : nullptr, d_image_offsets, n_images, n_rows_total,
                       d_track, d_track_len, consistent ? d_track_dup : nullptr, min_len, track_capacity, obs_capacity,
                       d_track_offsets, d_obs_row, d_obs_image, d_row_track, d_counts,
                       stream ? static_cast<hipStream_t>(stream) : h->stream);
    LF_HIP(h, hipGetLastError());
    return LF_MKD_OK;
}

int lf_mkd_gather_track_rows_device(lf_mkd *h, const void *d_src, uint32_t row_bytes, uint64_t n_rows_total,
                                    const int32_t *d_obs_row, const uint32_t *d_counts, uint64_t obs_capacity, void *d_dst,
                                    void *stream) {
    const auto at = [](const void *p) { return reinterpret_cast<uintptr_t>(p); };
    const char *msg = nullptr;
    if (!d_counts || (n_rows_total && !d_src) || (obs_capacity && (!d_obs_row || !d_dst))) msg = "null pointer";
    else if (row_bytes < 4 || row_bytes > 512 || (row_bytes & 3)) msg = "row_bytes must be a multiple of 4 in [4, 512]";
    else if ((at(d_src) | at(d_dst) | at(d_obs_row) | at(d_counts)) & 3) msg = "every array must be 4-byte aligned";
    else if (n_rows_total > kEdgeMax || obs_capacity > kEdgeMax) msg = "a total or a capacity above 2^31 - 1";
    else if (!h) msg = "null handle";
    if (msg) return q8_refuse(h, "gather_track_rows_device", msg);
    if (obs_capacity == 0) return LF_MKD_OK;
    LF_ENTER(h);
    launch_gather_track_rows(d_src, row_bytes, n_rows_total, d_obs_row, d_counts, obs_capacity, d_dst,
                             stream ? static_cast<hipStream_t>(stream) : h->stream);
    LF_HIP(h, hipGetLastError());
    return LF_MKD_OK;
}

// Link tables (csrc/mkd_link_table.hip).  Every refusal comes before the handle is looked at; the grid is tracks_link's.
static const char *link_table_sizes(uint64_t ea_capacity, uint32_t n_edges) {
    if (ea_capacity > kEdgeMax) return "a total or a capacity above 2^31 - 1";
    if (ea_capacity / link_table_plan(0, 0).slot_entries + n_edges > kEdgeMax)
        return "too many entries and edges for one call (the grid needs floor(ea_capacity / slot_entries) + n_edges workgroups, at "
               "most 2^31 - 1)";
    return nullptr;
}

int lf_mkd_link_table_plan(uint64_t ea_capacity, uint32_t n_edges, uint32_t *slot_entries, uint64_t *slots,
                           uint32_t *scan_fanout, uint32_t *scan_levels, uint64_t *scratch_bytes) {
    if (const char *msg = link_table_sizes(ea_capacity, n_edges)) return q8_refuse(nullptr, "link_table_plan", msg);
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
    const auto at = [](const void *p) { return reinterpret_cast<uintptr_t>(p); };
    const char *msg = nullptr;
    if (!d_image_offsets || !d_link_offsets || !d_counts) msg = "null pointer";
    else if (n_edges && (!d_edge_a || !d_edge_b)) msg = "null edge array";
    else if (n_edges && !d_edge_offsets_a) msg = "null layout array";
    else if (n_edges && !d_match) msg = "null match array";
    else if (link_capacity && (!d_link_a || !d_link_b)) msg = "null d_link_a or d_link_b";
    else if (flags & ~LF_MKD_LINK_TABLE_LOCAL) msg = "unknown flag bits";
    else if ((at(d_image_offsets) | at(d_edge_offsets_a) | at(d_link_offsets)) & 7) msg = "the offset arrays must be 8-byte aligned";
    else if ((at(d_edge_a) | at(d_edge_b) | at(d_match) | at(d_link_a) | at(d_link_b) | at(d_link_edge) | at(d_edge_links) |
              at(d_match_kept) | at(d_counts)) & 3)
        msg = "the edge, match, link and count arrays must be 4-byte aligned";
    else if (n_rows_total > kEdgeMax || link_capacity > kEdgeMax) msg = "a total or a capacity above 2^31 - 1";
    else if (!(msg = link_table_sizes(ea_capacity, n_edges)) && !h) msg = "null handle";
    if (msg) return q8_refuse(h, "link_table_device", msg);
    LF_ENTER(h);
    const LinkTablePlan plan = link_table_plan(ea_capacity, n_edges);
    if (plan.scratch_bytes)
        if (int rc = grow(h, h->d_link_table, plan.scratch_bytes)) return rc;
    launch_link_table(plan, plan.scratch_bytes ? h->d_link_table.get() : nullptr, d_image_offsets, n_images, n_rows_total, d_edge_a,
                      d_edge_b, d_edge_offsets_a, ea_capacity, n_edges, d_match, min_links, (flags & LF_MKD_LINK_TABLE_LOCAL) != 0,
                      link_capacity, d_link_offsets, d_link_a, d_link_b, d_link_edge, d_edge_links, d_match_kept, d_counts,
                      stream ? static_cast<hipStream_t>(stream) : h->stream);
    LF_HIP(h, hipGetLastError());
    return LF_MKD_OK;
}

// Candidate edges (csrc/mkd_select_edges.hip).  Every refusal comes before the handle is looked at.
static const char *select_edges_sizes(uint32_t n_a, uint32_t n_b, uint32_t k, uint64_t edge_capacity, uint32_t flags) {
    if (k == 0 || k > LF_MKD_SELECT_MAX_K) return "k must be in [1, 32]";
    if (flags & ~(LF_MKD_SELECT_SKIP_SELF | LF_MKD_SELECT_UNIQUE)) return "unknown flag bits";
    if ((flags & LF_MKD_SELECT_UNIQUE) && n_a != n_b) return "LF_MKD_SELECT_UNIQUE needs one pool (n_a == n_b)";
    if (n_a && n_b == 0) return "n_b == 0 with n_a > 0";
    if ((uint64_t)n_a * n_b > kEdgeMax) return "a table of more than 2^31 - 1 entries (n_a * n_b)";
    if ((uint64_t)n_a * k > kEdgeMax || edge_capacity > kEdgeMax) return "n_a * k or edge_capacity above 2^31 - 1";
    return nullptr;
}

int lf_mkd_select_edges_plan(uint32_t n_a, uint32_t n_b, uint32_t k, uint64_t edge_capacity, uint32_t flags,
                             uint32_t *compiled_k, uint32_t *rows_per_workgroup, uint64_t *workgroups, uint32_t *launches,
                             uint64_t *scratch_bytes) {
    if (const char *msg = select_edges_sizes(n_a, n_b, k, edge_capacity, flags)) return q8_refuse(nullptr, "select_edges_plan", msg);
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
    const auto at = [](const void *p) { return reinterpret_cast<uintptr_t>(p); };
    const char *msg = nullptr;
    if (n_a && !d_votes) msg = "null d_votes";
    else if (!d_counts) msg = "null d_counts";
    else if (edge_capacity && (!d_edge_a || !d_edge_b)) msg = "null d_edge_a or d_edge_b";
    else if ((at(d_votes) | at(d_rank) | at(d_rank_votes) | at(d_edge_a) | at(d_edge_b) | at(d_edge_votes) | at(d_counts)) & 3)
        msg = "every array must be 4-byte aligned";
    else if (!(msg = select_edges_sizes(n_a, n_b, k, edge_capacity, flags)) && !h) msg = "null handle";
    if (msg) return q8_refuse(h, "select_edges_device", msg);
    LF_ENTER(h);
    const SelectEdgesPlan plan = select_edges_plan(n_a, n_b, k, edge_capacity);
    if (plan.scratch_bytes)
        if (int rc = grow(h, h->d_select_edges, plan.scratch_bytes)) return rc;
    launch_select_edges(plan, plan.scratch_bytes ? h->d_select_edges.get() : nullptr, d_votes, n_a, n_b, k, min_votes,
                        (flags & LF_MKD_SELECT_SKIP_SELF) != 0, (flags & LF_MKD_SELECT_UNIQUE) != 0, edge_capacity, d_rank,
                        d_rank_votes, d_edge_a, d_edge_b, d_edge_votes, d_counts, stream ? static_cast<hipStream_t>(stream) : h->stream);
    LF_HIP(h, hipGetLastError());
    return LF_MKD_OK;
}

// Covisibility tables (csrc/mkd_covisibility.hip).  Every refusal comes before the handle is looked at.
static const char *covisibility_sizes(uint32_t n_images, uint64_t track_capacity, uint64_t obs_capacity, uint32_t flags) {
    if (flags & ~LF_MKD_COVIS_ACCUMULATE) return "unknown flag bits";
    if ((uint64_t)n_images * n_images > kEdgeMax) return "a table of more than 2^31 - 1 entries (n_images^2)";
    if (track_capacity > kEdgeMax || obs_capacity > kEdgeMax) return "track_capacity or obs_capacity above 2^31 - 1";
    return nullptr;
}

int lf_mkd_covisibility_plan(uint32_t n_images, uint64_t track_capacity, uint64_t obs_capacity, uint64_t n_edges, uint32_t flags,
                             uint32_t *form, uint64_t *workgroups, uint32_t *launches, uint64_t *scratch_bytes) {
    if (const char *msg = covisibility_sizes(n_images, track_capacity, obs_capacity, flags))
        return q8_refuse(nullptr, "covisibility_plan", msg);
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
    const auto at = [](const void *p) { return reinterpret_cast<uintptr_t>(p); };
    const char *msg = nullptr;
    if (n_images && !d_covis) msg = "null d_covis";
    else if (!d_table_counts) msg = "null d_table_counts";
    else if (!d_track_offsets) msg = "null d_track_offsets";
    else if (obs_capacity && !d_obs_image) msg = "null d_obs_image";
    else if (!d_edge_a != !d_edge_b) msg = "only one of d_edge_a and d_edge_b";
    else if (n_edges && !d_edge_a) msg = "n_edges > 0 without d_edge_a and d_edge_b";
    else if (at(d_track_offsets) & 7) msg = "d_track_offsets must be 8-byte aligned";
    else if ((at(d_obs_image) | at(d_table_counts) | at(d_edge_a) | at(d_edge_b) | at(d_covis)) & 3)
        msg = "the observation, count, edge and table arrays must be 4-byte aligned";
    else if (!(msg = covisibility_sizes(n_images, track_capacity, obs_capacity, flags)) && !h) msg = "null handle";
    if (msg) return q8_refuse(h, "covisibility_device", msg);
    if (n_images == 0) return LF_MKD_OK;
    LF_ENTER(h);
    const CovisibilityPlan plan = covisibility_plan(n_images, track_capacity, obs_capacity, n_edges);
    if (plan.scratch_bytes)
        if (int rc = grow(h, h->d_covisibility, plan.scratch_bytes)) return rc;
    launch_covisibility(plan, plan.scratch_bytes ? h->d_covisibility.get() : nullptr, d_track_offsets, track_capacity,
                        d_obs_image, obs_capacity, d_table_counts, n_images, d_edge_a, d_edge_b, n_edges,
                        (flags & LF_MKD_COVIS_ACCUMULATE) != 0, d_covis, stream ? static_cast<hipStream_t>(stream) : h->stream);
    LF_HIP(h, hipGetLastError());
    return LF_MKD_OK;
}

// Two-view poses (csrc/mkd_two_view_pose.hip).  Every refusal comes before the handle is looked at.  The cosine of the
// parallax threshold is formed here, once, in double: no transcendental runs on the device (tests/cpp/pose_twin.cpp forms it
// with the same expression).
static const char *two_view_pose_scalars(float min_parallax_deg, uint32_t flags) {
    if (flags) return "unknown flag bits (no flag is defined: flags must be 0)";
    if (!(min_parallax_deg >= 0.f && min_parallax_deg <= 180.f)) return "min_parallax_deg must be in [0, 180]";
    return nullptr;
}

int lf_mkd_two_view_pose_device(lf_mkd *h, const lf_mkd_keypoint *d_kps, uint64_t n_rows_total, const uint32_t *d_edge_a,
                                const uint32_t *d_edge_b, uint32_t n_edges, const float *d_intrinsics, uint32_t n_images,
                                const float *d_F, const uint64_t *d_link_offsets, const int32_t *d_link_a, const int32_t *d_link_b,
                                uint64_t link_capacity, float min_parallax_deg, uint32_t flags, float *d_R, float *d_t,
                                uint32_t *d_stats, float *d_sigma, float *d_points, void *stream) {
    const auto at = [](const void *p) { return reinterpret_cast<uintptr_t>(p); };
    const char *msg = nullptr;
    if (n_edges && (!d_edge_a || !d_edge_b)) msg = "null edge array";
    else if (n_edges && (!d_F || !d_link_offsets || !d_R || !d_t || !d_stats)) msg = "null d_F, d_link_offsets, d_R, d_t or d_stats";
    else if (n_edges && n_images && !d_intrinsics) msg = "null d_intrinsics";
    else if (n_edges && link_capacity && (!d_link_a || !d_link_b)) msg = "null d_link_a or d_link_b";
    else if (n_edges && link_capacity && n_rows_total && !d_kps) msg = "null d_kps";
    else if ((msg = two_view_pose_scalars(min_parallax_deg, flags))) {}
    else if (at(d_link_offsets) & 7) msg = "d_link_offsets must be 8-byte aligned";
    else if ((at(d_kps) | at(d_edge_a) | at(d_edge_b) | at(d_intrinsics) | at(d_F) | at(d_link_a) | at(d_link_b) | at(d_R) |
              at(d_t) | at(d_stats) | at(d_sigma) | at(d_points)) & 3)
        msg = "the keypoint, edge, intrinsics, model, link and output arrays must be 4-byte aligned";
    else if (n_rows_total > kEdgeMax || link_capacity > kEdgeMax || n_edges > kEdgeMax)
        msg = "a total or a capacity above 2^31 - 1";
    else if (!h) msg = "null handle";
    if (msg) return q8_refuse(h, "two_view_pose_device", msg);
    if (n_edges == 0) return LF_MKD_OK;
    LF_ENTER(h);
    const double cmin = std::cos(double(min_parallax_deg) * (3.14159265358979323846 / 180.0));
    launch_two_view_pose(reinterpret_cast<const float *>(d_kps), n_rows_total, d_edge_a, d_edge_b, n_edges, d_intrinsics, n_images,
                         d_F, d_link_offsets, d_link_a, d_link_b, link_capacity, cmin, d_R, d_t, d_stats, d_sigma, d_points,
                         stream ? static_cast<hipStream_t>(stream) : h->stream);
    LF_HIP(h, hipGetLastError());
    return LF_MKD_OK;
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
    else if (na > kEdgeMax || nb > kEdgeMax || na + nb > kEdgeMax) msg = "more than 2^31 - 1 rows";
    else if (!h) msg = "null handle";
    if (msg) return q8_refuse(h, "two_view_pose", msg);
    LF_ENTER(h);
    std::vector<int32_t> links;   // a's rows, then b's
    for (uint64_t i = 0; i < na; ++i)
        if (match[i] >= 0 && uint64_t(match[i]) < nb) links.push_back(int32_t(i));
    const uint64_t n_links = links.size();
    links.resize(2 * n_links);
    for (uint64_t k = 0; k < n_links; ++k) links[n_links + k] = int32_t(na + uint64_t(match[links[k]]));
    auto up16 = [](uint64_t b) { return (std::max<uint64_t>(b, 1) + 15) / 16 * 16; };
    // offsets [2] u64, edge a, edge b, K [2][4], F [9], then the outputs R [9], t [3], stats [4], sigma [3], then the arrays
    const uint64_t o_off = 0, o_ea = 16, o_eb = 32, o_k = 48, o_f = 80, o_r = 128, o_t = 176, o_st = 192, o_sg = 208, o_kps = 224,
                   o_la = o_kps + up16((na + nb) * sizeof(lf_mkd_keypoint)), o_lb = o_la + up16(n_links * 4),
                   o_pt = o_lb + up16(n_links * 4), total = o_pt + up16(points ? n_links * 16 : 0);
    if (int rc = grow(h, h->d_ver_io, total)) return rc;
    unsigned char *io = h->d_ver_io;
    const uint64_t offs[2] = {0, n_links};
    const uint32_t ea = 0, eb = 1;
    float K[8];
    for (int i = 0; i < 4; ++i) K[i] = Ka[i], K[4 + i] = Kb[i];
    LF_HIP(h, hipMemcpyAsync(io + o_off, offs, sizeof(offs), hipMemcpyHostToDevice, h->stream));
    LF_HIP(h, hipMemcpyAsync(io + o_ea, &ea, 4, hipMemcpyHostToDevice, h->stream));
    LF_HIP(h, hipMemcpyAsync(io + o_eb, &eb, 4, hipMemcpyHostToDevice, h->stream));
    LF_HIP(h, hipMemcpyAsync(io + o_k, K, sizeof(K), hipMemcpyHostToDevice, h->stream));
    LF_HIP(h, hipMemcpyAsync(io + o_f, F, 9 * sizeof(float), hipMemcpyHostToDevice, h->stream));
    if (na) LF_HIP(h, hipMemcpyAsync(io + o_kps, kps_a, na * sizeof(lf_mkd_keypoint), hipMemcpyHostToDevice, h->stream));
    if (nb)
        LF_HIP(h, hipMemcpyAsync(io + o_kps + na * sizeof(lf_mkd_keypoint), kps_b, nb * sizeof(lf_mkd_keypoint),
                                 hipMemcpyHostToDevice, h->stream));
    if (n_links) {
        LF_HIP(h, hipMemcpyAsync(io + o_la, links.data(), n_links * 4, hipMemcpyHostToDevice, h->stream));
        LF_HIP(h, hipMemcpyAsync(io + o_lb, links.data() + n_links, n_links * 4, hipMemcpyHostToDevice, h->stream));
    }
    if (int rc = lf_mkd_two_view_pose_device(
            h, reinterpret_cast<const lf_mkd_keypoint *>(io + o_kps), na + nb, reinterpret_cast<const uint32_t *>(io + o_ea),
            reinterpret_cast<const uint32_t *>(io + o_eb), 1, reinterpret_cast<const float *>(io + o_k), 2,
            reinterpret_cast<const float *>(io + o_f), reinterpret_cast<const uint64_t *>(io + o_off),
            reinterpret_cast<const int32_t *>(io + o_la), reinterpret_cast<const int32_t *>(io + o_lb), n_links, min_parallax_deg,
            flags, reinterpret_cast<float *>(io + o_r), reinterpret_cast<float *>(io + o_t), reinterpret_cast<uint32_t *>(io + o_st),
            reinterpret_cast<float *>(io + o_sg), points ? reinterpret_cast<float *>(io + o_pt) : nullptr, h->stream))
        return rc;
    std::vector<float> link_points(points ? 4 * n_links : 0);
    LF_HIP(h, hipMemcpyAsync(R, io + o_r, 9 * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    LF_HIP(h, hipMemcpyAsync(t, io + o_t, 3 * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    LF_HIP(h, hipMemcpyAsync(stats, io + o_st, 4 * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    if (sigma) LF_HIP(h, hipMemcpyAsync(sigma, io + o_sg, 3 * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    if (points && n_links)
        LF_HIP(h, hipMemcpyAsync(link_points.data(), io + o_pt, n_links * 16, hipMemcpyDeviceToHost, h->stream));
    LF_HIP(h, hipStreamSynchronize(h->stream));
    if (points) {
        for (uint64_t i = 0; i < na; ++i) points[4 * i] = points[4 * i + 1] = points[4 * i + 2] = 0.f, points[4 * i + 3] = 2.f;
        for (uint64_t k = 0; k < n_links; ++k) std::memcpy(points + 4 * uint64_t(links[k]), link_points.data() + 4 * k, 16);
    }
    return LF_MKD_OK;
}

// Track triangulation (csrc/mkd_triangulate.hip).  Every refusal comes before the handle is looked at.  The squared threshold
// is formed here, once, in double (tests/cpp/triangulate_twin.cpp forms it with the same expression).
static const char *triangulate_scalars(float max_reproj_px, uint32_t rounds, uint32_t flags) {
    if (flags) return "unknown flag bits (no flag is defined: flags must be 0)";
    if (!(max_reproj_px > 0.f) || !std::isfinite(max_reproj_px)) return "max_reproj_px must be finite and positive";
    if (rounds > 4) return "rounds must be 0 .. 4";
    return nullptr;
}

int lf_mkd_triangulate_tracks_device(lf_mkd *h, const lf_mkd_keypoint *d_kps, uint64_t n_rows_total, const uint64_t *d_track_offsets,
                                     uint64_t track_capacity, const int32_t *d_obs_row, const uint32_t *d_obs_image,
                                     uint64_t obs_capacity, const uint32_t *d_table_counts, const float *d_intrinsics,
                                     const float *d_poses, uint32_t n_images, float max_reproj_px, uint32_t rounds, uint32_t flags,
                                     float *d_points, uint32_t *d_stats, float *d_err, uint32_t *d_obs_state, void *stream) {
    const auto at = [](const void *p) { return reinterpret_cast<uintptr_t>(p); };
    const char *msg = nullptr;
    if (track_capacity && (!d_track_offsets || !d_table_counts || !d_points || !d_stats))
        msg = "null d_track_offsets, d_table_counts, d_points or d_stats";
    else if (track_capacity && obs_capacity && (!d_obs_row || !d_obs_image)) msg = "null d_obs_row or d_obs_image";
    else if (track_capacity && obs_capacity && n_rows_total && !d_kps) msg = "null d_kps";
    else if (track_capacity && obs_capacity && n_images && (!d_intrinsics || !d_poses)) msg = "null d_intrinsics or d_poses";
    else if ((msg = triangulate_scalars(max_reproj_px, rounds, flags))) {}
    else if (at(d_track_offsets) & 7) msg = "d_track_offsets must be 8-byte aligned";
    else if ((at(d_kps) | at(d_obs_row) | at(d_obs_image) | at(d_table_counts) | at(d_intrinsics) | at(d_poses) | at(d_points) |
              at(d_stats) | at(d_err) | at(d_obs_state)) & 3)
        msg = "the keypoint, observation, count, intrinsics, pose and output arrays must be 4-byte aligned";
    else if (n_rows_total > kEdgeMax || track_capacity > kEdgeMax || obs_capacity > kEdgeMax)
        msg = "a total or a capacity above 2^31 - 1";
    else if (!h) msg = "null handle";
    if (msg) return q8_refuse(h, "triangulate_tracks_device", msg);
    if (track_capacity == 0) return LF_MKD_OK;
    LF_ENTER(h);
    const double thr2 = double(max_reproj_px) * double(max_reproj_px);
    launch_triangulate_tracks(reinterpret_cast<const float *>(d_kps), n_rows_total, d_track_offsets, track_capacity, d_obs_row,
                              d_obs_image, obs_capacity, d_table_counts, d_intrinsics, d_poses, n_images, thr2, rounds, d_points,
                              d_stats, d_err, d_obs_state, stream ? static_cast<hipStream_t>(stream) : h->stream);
    LF_HIP(h, hipGetLastError());
    return LF_MKD_OK;
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
    else if (n_rows_total > kEdgeMax || n_tracks > kEdgeMax || n_obs > kEdgeMax) msg = "a total above 2^31 - 1";
    else if (!h) msg = "null handle";
    if (msg) return q8_refuse(h, "triangulate_tracks", msg);
    if (n_tracks == 0) return LF_MKD_OK;
    LF_ENTER(h);
    auto up16 = [](uint64_t b) { return (std::max<uint64_t>(b, 1) + 15) / 16 * 16; };
    const uint64_t o_cnt = 0, o_off = 16, o_kps = o_off + up16((n_tracks + 1) * 8),
                   o_row = o_kps + up16(n_rows_total * sizeof(lf_mkd_keypoint)), o_img = o_row + up16(n_obs * 4),
                   o_k = o_img + up16(n_obs * 4), o_p = o_k + up16(uint64_t(n_images) * 16),
                   o_pt = o_p + up16(uint64_t(n_images) * 48), o_st = o_pt + up16(n_tracks * 16), o_err = o_st + up16(n_tracks * 16),
                   o_os = o_err + up16(err ? n_tracks * 8 : 0), total = o_os + up16(obs_state ? n_obs * 4 : 0);
    if (int rc = grow(h, h->d_ver_io, total)) return rc;
    unsigned char *io = h->d_ver_io;
    // (counts saturate: the totals are below 2^31)
    const uint32_t cnt[2] = {uint32_t(n_tracks), uint32_t(n_obs)};
    const auto up = [&](uint64_t at_, const void *src, uint64_t bytes) {
        return bytes ? hipMemcpyAsync(io + at_, src, bytes, hipMemcpyHostToDevice, h->stream) : hipSuccess;
    };
    const auto down = [&](void *dst, uint64_t at_, uint64_t bytes) {
        return bytes ? hipMemcpyAsync(dst, io + at_, bytes, hipMemcpyDeviceToHost, h->stream) : hipSuccess;
    };
    LF_HIP(h, up(o_cnt, cnt, sizeof(cnt)));
    LF_HIP(h, up(o_off, track_offsets, (n_tracks + 1) * 8));
    LF_HIP(h, up(o_kps, kps, n_obs ? n_rows_total * sizeof(lf_mkd_keypoint) : 0));
    LF_HIP(h, up(o_row, obs_row, n_obs * 4));
    LF_HIP(h, up(o_img, obs_image, n_obs * 4));
    LF_HIP(h, up(o_k, intrinsics, n_obs ? uint64_t(n_images) * 16 : 0));
    LF_HIP(h, up(o_p, poses, n_obs ? uint64_t(n_images) * 48 : 0));
    if (obs_state) LF_HIP(h, up(o_os, obs_state, n_obs * 4));
    if (int rc = lf_mkd_triangulate_tracks_device(
            h, reinterpret_cast<const lf_mkd_keypoint *>(io + o_kps), n_rows_total, reinterpret_cast<const uint64_t *>(io + o_off),
            n_tracks, reinterpret_cast<const int32_t *>(io + o_row), reinterpret_cast<const uint32_t *>(io + o_img), n_obs,
            reinterpret_cast<const uint32_t *>(io + o_cnt), reinterpret_cast<const float *>(io + o_k),
            reinterpret_cast<const float *>(io + o_p), n_images, max_reproj_px, rounds, flags, reinterpret_cast<float *>(io + o_pt),
            reinterpret_cast<uint32_t *>(io + o_st), err ? reinterpret_cast<float *>(io + o_err) : nullptr,
            obs_state ? reinterpret_cast<uint32_t *>(io + o_os) : nullptr, h->stream))
        return rc;
    LF_HIP(h, down(points, o_pt, n_tracks * 16));
    LF_HIP(h, down(stats, o_st, n_tracks * 16));
    if (err) LF_HIP(h, down(err, o_err, n_tracks * 8));
    if (obs_state) LF_HIP(h, down(obs_state, o_os, n_obs * 4));
    LF_HIP(h, hipStreamSynchronize(h->stream));
    return LF_MKD_OK;
}

// Camera resection (csrc/mkd_resect.hip).  Every refusal comes before the handle is looked at.  The squared threshold and the
// parallax cosine are formed here, once, in double (tests/cpp/resect_twin.cpp forms them with the same expressions).
static const char *resect_scalars(float max_reproj_px, float min_parallax_deg, uint32_t n_samples, uint32_t rounds, uint32_t flags) {
    if (flags & ~uint32_t(LF_MKD_RESECT_ALL)) return "unknown flag bits";
    if (!(max_reproj_px > 0.f) || !std::isfinite(max_reproj_px)) return "max_reproj_px must be finite and positive";
    if (!(min_parallax_deg >= 0.f && min_parallax_deg <= 180.f)) return "min_parallax_deg must be in [0, 180]";
    if (n_samples < 1 || n_samples > 4096) return "n_samples must be 1 .. 4096";
    if (rounds > 4) return "rounds must be 0 .. 4";
    return nullptr;
}

int lf_mkd_resect_cameras_device(lf_mkd *h, const lf_mkd_keypoint *d_kps, const uint64_t *d_image_offsets, uint32_t n_images,
                                 uint64_t n_rows_total, const int32_t *d_row_track, const float *d_points, uint64_t track_capacity,
                                 const uint32_t *d_table_counts, const float *d_intrinsics, const float *d_poses,
                                 float max_reproj_px, float min_parallax_deg, uint32_t n_samples, uint32_t min_inliers,
                                 uint32_t rounds, uint32_t seed, uint32_t flags, float *d_poses_out, uint32_t *d_stats, float *d_err,
                                 uint32_t *d_row_state, void *stream) {
    const auto at = [](const void *p) { return reinterpret_cast<uintptr_t>(p); };
    const char *msg = nullptr;
    if (n_images && (!d_image_offsets || !d_table_counts || !d_intrinsics || !d_poses || !d_poses_out || !d_stats))
        msg = "null d_image_offsets, d_table_counts, d_intrinsics, d_poses, d_poses_out or d_stats";
    else if (n_images && n_rows_total && (!d_kps || !d_row_track)) msg = "null d_kps or d_row_track";
    else if (n_images && n_rows_total && track_capacity && !d_points) msg = "null d_points";
    else if ((msg = resect_scalars(max_reproj_px, min_parallax_deg, n_samples, rounds, flags))) {}
    else if (at(d_image_offsets) & 7) msg = "d_image_offsets must be 8-byte aligned";
    else if ((at(d_kps) | at(d_row_track) | at(d_points) | at(d_table_counts) | at(d_intrinsics) | at(d_poses) | at(d_poses_out) |
              at(d_stats) | at(d_err) | at(d_row_state)) & 3)
        msg = "the keypoint, track, point, count, intrinsics, pose and output arrays must be 4-byte aligned";
    else if (n_images > kEdgeMax || n_rows_total > kEdgeMax || track_capacity > kEdgeMax)
        msg = "n_images, n_rows_total or track_capacity above 2^31 - 1";
    else if (!h) msg = "null handle";
    if (msg) return q8_refuse(h, "resect_cameras_device", msg);
    if (n_images == 0) return LF_MKD_OK;
    LF_ENTER(h);
    if (int rc = grow(h, h->d_resect, resect_scratch_bytes(n_images, n_rows_total, n_samples))) return rc;
    const double thr2 = double(max_reproj_px) * double(max_reproj_px);
    const double cmin = std::cos(double(min_parallax_deg) * (3.14159265358979323846 / 180.0));
    launch_resect_cameras(h->d_resect.get(), reinterpret_cast<const float *>(d_kps), d_image_offsets, n_images, n_rows_total,
                          d_row_track, d_points, track_capacity, d_table_counts, d_intrinsics, d_poses, thr2, cmin, n_samples,
                          min_inliers, rounds, seed, (flags & LF_MKD_RESECT_ALL) != 0, d_poses_out, d_stats, d_err, d_row_state,
                          stream ? static_cast<hipStream_t>(stream) : h->stream);
    LF_HIP(h, hipGetLastError());
    return LF_MKD_OK;
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
    else if (n_rows > kEdgeMax || n_tracks > kEdgeMax) msg = "a total above 2^31 - 1";
    else if (!h) msg = "null handle";
    if (msg) return q8_refuse(h, "resect_camera", msg);
    LF_ENTER(h);
    auto up16 = [](uint64_t b) { return (std::max<uint64_t>(b, 1) + 15) / 16 * 16; };
    const uint64_t o_off = 0, o_cnt = 16, o_k = 32, o_p = 48, o_po = 96, o_st = 144, o_err = 160, o_kps = 176,
                   o_rt = o_kps + up16(n_rows * sizeof(lf_mkd_keypoint)), o_pt = o_rt + up16(n_rows * 4),
                   o_rs = o_pt + up16(n_tracks * 16), total = o_rs + up16(row_state ? n_rows * 4 : 0);
    if (int rc = grow(h, h->d_ver_io, total)) return rc;
    unsigned char *io = h->d_ver_io;
    const uint64_t off[2] = {0, n_rows};
    const uint32_t cnt[2] = {uint32_t(n_tracks), 0};
    const float zero[12] = {};
    const auto up = [&](uint64_t at_, const void *src, uint64_t bytes) {
        return bytes ? hipMemcpyAsync(io + at_, src, bytes, hipMemcpyHostToDevice, h->stream) : hipSuccess;
    };
    const auto down = [&](void *dst, uint64_t at_, uint64_t bytes) {
        return bytes ? hipMemcpyAsync(dst, io + at_, bytes, hipMemcpyDeviceToHost, h->stream) : hipSuccess;
    };
    LF_HIP(h, up(o_off, off, sizeof(off)));
    LF_HIP(h, up(o_cnt, cnt, sizeof(cnt)));
    LF_HIP(h, up(o_k, intrinsics, 16));
    LF_HIP(h, up(o_p, zero, sizeof(zero)));
    LF_HIP(h, up(o_kps, kps, n_rows * sizeof(lf_mkd_keypoint)));
    LF_HIP(h, up(o_rt, row_track, n_rows * 4));
    LF_HIP(h, up(o_pt, points, n_rows ? n_tracks * 16 : 0));
    if (row_state) LF_HIP(h, up(o_rs, row_state, n_rows * 4));
    // (the staged copies are pageable: they have left the host arrays when the calls return)
    if (int rc = lf_mkd_resect_cameras_device(
            h, reinterpret_cast<const lf_mkd_keypoint *>(io + o_kps), reinterpret_cast<const uint64_t *>(io + o_off), 1, n_rows,
            reinterpret_cast<const int32_t *>(io + o_rt), reinterpret_cast<const float *>(io + o_pt), n_tracks,
            reinterpret_cast<const uint32_t *>(io + o_cnt), reinterpret_cast<const float *>(io + o_k),
            reinterpret_cast<const float *>(io + o_p), max_reproj_px, min_parallax_deg, n_samples, min_inliers, rounds, seed, flags,
            reinterpret_cast<float *>(io + o_po), reinterpret_cast<uint32_t *>(io + o_st), reinterpret_cast<float *>(io + o_err),
            row_state ? reinterpret_cast<uint32_t *>(io + o_rs) : nullptr, h->stream))
        return rc;
    LF_HIP(h, down(pose, o_po, 48));
    LF_HIP(h, down(stats, o_st, 16));
    if (err) LF_HIP(h, down(err, o_err, 8));
    if (row_state) LF_HIP(h, down(row_state, o_rs, n_rows * 4));
    LF_HIP(h, hipStreamSynchronize(h->stream));
    return LF_MKD_OK;
}

// Guided matching over 8-bit rows: the two calls' refusals together, the q8 pairs call's grid.
int lf_mkd_match_q8_guided_pairs_device(lf_mkd *h, const uint8_t *d_a, const lf_mkd_keypoint *d_kps_a, const uint64_t *d_offsets_a,
                                        uint64_t na_total, const uint8_t *d_b, const lf_mkd_keypoint *d_kps_b,
                                        const uint64_t *d_offsets_b, uint64_t nb_total, const float *d_model, uint32_t n_pairs,
                                        uint32_t kind, float threshold_px, float ratio, uint32_t flags, int32_t *d_match_ab,
                                        int32_t *d_match_ba, int32_t *d_best, int32_t *d_second, void *stream) {
    const bool mutual = flags & LF_MKD_MATCH_MUTUAL;
    const char *msg = nullptr;
    if (!d_a || !d_b || !d_kps_a || !d_kps_b || !d_offsets_a || !d_offsets_b || !d_model || !d_match_ab) msg = "null pointer";
    else if (flags & ~LF_MKD_MATCH_MUTUAL) msg = "unknown flag bits";
    else if (mutual && !d_match_ba) msg = "LF_MKD_MATCH_MUTUAL needs d_match_ba";
    else if (kind > LF_MKD_GUIDE_FUNDAMENTAL) msg = "kind must be LF_MKD_GUIDE_HOMOGRAPHY or LF_MKD_GUIDE_FUNDAMENTAL";
    // (the verifiers' rule, verify_args below: the kernel compares against thr^2 in f32)
    else if (!(threshold_px > 0.f) || !std::isnormal(threshold_px * threshold_px))
        msg = "threshold_px must be positive, with a finite normal f32 square (about 1.09e-19 .. 1.84e19)";
    else if ((reinterpret_cast<uintptr_t>(d_a) | reinterpret_cast<uintptr_t>(d_b)) & 15) msg = "d_a and d_b must be 16-byte aligned";
    else if (!(msg = match_q8_pairs_sizes(na_total, nb_total, n_pairs, d_match_ba != nullptr)) && !h) msg = "null handle";
    if (msg) return q8_refuse(h, "match_q8_guided_pairs_device", msg);
    if (n_pairs == 0) return LF_MKD_OK;
    LF_ENTER(h);
    launch_match_q8_guided_pairs(d_a, reinterpret_cast<const float *>(d_kps_a), d_offsets_a, na_total, d_b,
                                 reinterpret_cast<const float *>(d_kps_b), d_offsets_b, nb_total, d_model, n_pairs, kind,
                                 threshold_px, ratio, mutual, d_match_ab, d_match_ba, d_best, d_second,
                                 stream ? static_cast<hipStream_t>(stream) : h->stream);
    LF_HIP(h, hipGetLastError());
    return LF_MKD_OK;
}

// The arguments of both verification entry points, checked before the handle so that every bad argument is reported without
// a device: the message goes to the handle, or to lf_mkd_last_error(NULL) when there is none.
static int verify_args(lf_mkd *h, bool null_pointer, uint32_t n_hypotheses, float threshold_px, const char *what) {
    std::string msg;
    if (null_pointer) msg = ": null pointer";
    else if (n_hypotheses == 0 || n_hypotheses > 65536) msg = ": n_hypotheses must be 1 .. 65536";
    // the kernels compare against thr^2 in f32: it must be a normal number (thr of about 1.09e-19 .. 1.84e19), else an exact
    // match is no inlier (thr^2 = 0) or every refit is kept (thr^2 = inf)
    else if (!(threshold_px > 0.f) || !std::isnormal(threshold_px * threshold_px))
        msg = ": threshold_px must be positive, with a finite normal f32 square (about 1.09e-19 .. 1.84e19)";
    else if (!h) msg = ": null handle";
    if (msg.empty()) return LF_MKD_OK;
    (h ? h->err : g_create_error) = what + msg;
    return LF_MKD_ERR_BAD_ARG;
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
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : h->stream;
    launch(reinterpret_cast<const float *>(d_kps_a), d_offsets_a, reinterpret_cast<const float *>(d_kps_b), d_offsets_b, d_match,
           n_pairs, n_hypotheses, threshold_px, seed, flags, slices, h->d_ver_pairs, h->d_ver_counts, d_model, d_verified,
           d_stats, s);
    LF_HIP(h, hipGetLastError());
    return LF_MKD_OK;
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
    if (na > 0x7FFFFFFFull || nb > 0x7FFFFFFFull) return fail(h, LF_MKD_ERR_BAD_ARG, std::string(what) + ": more than 2^31 - 1 rows");
    LF_ENTER(h);
    // one staging array, every part 16-byte aligned: offsets, keypoints of a and b, match, then the outputs
    auto up16 = [](uint64_t b) { return (std::max<uint64_t>(b, 1) + 15) / 16 * 16; };   // (empty parts do not share an address)
    const uint64_t o_off = 0, o_ka = 64, o_kb = o_ka + up16(na * sizeof(lf_mkd_keypoint)),
                   o_m = o_kb + up16(nb * sizeof(lf_mkd_keypoint)), o_v = o_m + up16(na * 4), o_h = o_v + up16(na * 4),
                   o_st = o_h + 48, total = o_st + 16;
    if (int rc = grow(h, h->d_ver_io, total)) return rc;
    unsigned char *io = h->d_ver_io;
    const uint64_t offs[4] = {0, na, 0, nb};
    LF_HIP(h, hipMemcpyAsync(io + o_off, offs, sizeof(offs), hipMemcpyHostToDevice, h->stream));
    if (na) LF_HIP(h, hipMemcpyAsync(io + o_ka, kps_a, na * sizeof(lf_mkd_keypoint), hipMemcpyHostToDevice, h->stream));
    if (nb) LF_HIP(h, hipMemcpyAsync(io + o_kb, kps_b, nb * sizeof(lf_mkd_keypoint), hipMemcpyHostToDevice, h->stream));
    if (na) LF_HIP(h, hipMemcpyAsync(io + o_m, match, na * 4, hipMemcpyHostToDevice, h->stream));
    const uint64_t *d_offs = reinterpret_cast<const uint64_t *>(io + o_off);
    if (int rc = device(h, reinterpret_cast<const lf_mkd_keypoint *>(io + o_ka), d_offs,
                        reinterpret_cast<const lf_mkd_keypoint *>(io + o_kb), d_offs + 2, reinterpret_cast<const int32_t *>(io + o_m),
                        1, n_hypotheses, threshold_px, seed, flags, reinterpret_cast<float *>(io + o_h),
                        reinterpret_cast<int32_t *>(io + o_v), reinterpret_cast<uint32_t *>(io + o_st), h->stream))
        return rc;
    LF_HIP(h, hipMemcpyAsync(model, io + o_h, 9 * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    LF_HIP(h, hipMemcpyAsync(stats, io + o_st, 4 * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    if (na) LF_HIP(h, hipMemcpyAsync(verified, io + o_v, na * 4, hipMemcpyDeviceToHost, h->stream));
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
