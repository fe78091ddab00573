// The handle behind the C ABI (include/lf_mkd.h) and what owns its memory: shared by the translation units of the entry
// layer -- lf_mkd.cpp, lf_mkd_match.cpp, lf_mkd_tables.cpp, lf_mkd_geometry.cpp -- and by nobody else.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <utility>
#include <vector>

#include "lf_mkd_internal.h"
#include "mkd_device.h"

namespace lfmkd {

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

}  // namespace lfmkd

using namespace lfmkd;   // (a private header: every file that includes it is written in this namespace)

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
    // lf_mkd_bundle_adjust_device's scratch (bundle_scratch_bytes), in the same way; lf_mkd_bundle_adjust_intrinsics_device's
    // too (bundle_intrinsics_scratch_bytes: the same layout with the groups' arrays behind it)
    HipArray<unsigned char> d_bundle;
    // lf_mkd_view_graph_device's scratch (view_graph_plan's scratch_bytes), in the same way
    HipArray<unsigned char> d_view_graph;
    // lf_mkd_global_positions_device's scratch (global_positions_plan's scratch_bytes), in the same way
    HipArray<unsigned char> d_positions;
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

namespace lfmkd {

// lf_mkd_last_error(NULL): what went wrong where there is no handle to keep the message (per thread; lf_mkd.cpp)
extern thread_local std::string g_create_error;

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

inline int fail(lf_mkd *h, int code, const std::string &msg) {
    if (h) h->err = msg;
    return code;
}

// the stream a call runs on: the caller's, or the handle's own
inline hipStream_t stream_of(const lf_mkd *h, void *stream) { return stream ? static_cast<hipStream_t>(stream) : h->stream; }

// how a device form ends: what its launches left behind
inline int launched(lf_mkd *h) {
    LF_HIP(h, hipGetLastError());
    return LF_MKD_OK;
}

// A recorded pipeline holds raw pointers into the scratch buffers: re-allocating one of them retires the recordings
// (lf_mkd_stream_frame then asks for a new lf_mkd_stream_create instead of touching freed memory, and lf_mkd_detect records anew).
inline void retire_graph(lf_mkd *h) {
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

}  // namespace lfmkd
