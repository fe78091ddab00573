// The entry layer's vocabulary: how a call's arguments are refused, the rules several calls share, and the staging of the
// host forms.  Every refusal of the calls written with it comes before the handle is looked at, so that a bad argument is
// reported without a device: the message goes to the handle, or to lf_mkd_last_error(NULL) when there is none, and a null
// handle is the last fault a call reports.  The order of a call's checks is part of its contract
// (tests/test_refusal_transcript.py).
#pragma once
#include <cmath>
#include <cstdint>

#include "lf_mkd_handle.h"

namespace lfmkd {

// The one way to report LF_MKD_ERR_BAD_ARG before a device is touched.
inline int refuse(lf_mkd *h, const char *who, const char *msg) {
    (h ? h->err : g_create_error) = std::string(who) + ": " + msg;
    return LF_MKD_ERR_BAD_ARG;
}

// Is one of the addresses not a multiple of mask + 1?  (A null pointer is aligned.)
template <typename... P>
bool misaligned(uintptr_t mask, const P *...p) {
    return ((reinterpret_cast<uintptr_t>(p) | ... | uintptr_t(0)) & mask) != 0;
}

// Rows, entries and workgroups are indexed in 32 bits, signed where -1 means "none": nothing counts past 2^31 - 1.
constexpr uint64_t kRowMax = 0x7FFFFFFFull;
template <typename... N>
bool above(uint64_t max, N... n) {
    return ((uint64_t(n) > max) || ...);
}

// A launch's scratch of `bytes` (its plan's scratch_bytes) in one of the handle's arrays: nullptr when it needs none.
inline int scratch(lf_mkd *h, HipArray<unsigned char> &buf, uint64_t bytes, unsigned char **p) {
    *p = nullptr;
    if (bytes == 0) return LF_MKD_OK;
    if (int rc = grow(h, buf, bytes)) return rc;
    *p = buf.get();
    return LF_MKD_OK;
}

// ---- rules shared by several calls: the message, or nullptr -----------------------------------------------------------------
// The verifiers and the guided matchers compare against thr^2 in f32: it must be a normal number (thr of about 1.09e-19 ..
// 1.84e19), else an exact match is no inlier (thr^2 = 0) or every refit is kept (thr^2 = inf).
inline const char *threshold_rule(float threshold_px) {
    return threshold_px > 0.f && std::isnormal(threshold_px * threshold_px)
               ? nullptr
               : "threshold_px must be positive, with a finite normal f32 square (about 1.09e-19 .. 1.84e19)";
}
inline const char *parallax_rule(float min_parallax_deg) {
    return min_parallax_deg >= 0.f && min_parallax_deg <= 180.f ? nullptr : "min_parallax_deg must be in [0, 180]";
}
inline const char *reproj_rule(float max_reproj_px) {
    return max_reproj_px > 0.f && std::isfinite(max_reproj_px) ? nullptr : "max_reproj_px must be finite and positive";
}
inline const char *rounds_rule(uint32_t rounds) { return rounds > 4 ? "rounds must be 0 .. 4" : nullptr; }
// The quantiser's scale (the 8-bit calls and the track descriptors): 0 -> the default; nullptr: fine.
inline const char *q8_scale(float &scale) {
    if (scale == 0.f) scale = 256.f;
    return scale > 0.f && std::isnormal(scale) ? nullptr : "scale must be a positive, finite, normal f32 (0: the default, 256)";
}
// The scalars of lf_mkd_track_descriptors_device and of its host form (the states are triangulation's: 0, 1, 2).
inline const char *track_desc_scalars(uint32_t min_state, float min_parallax_deg, float &scale) {
    if (min_state > 2) return "min_state must be 0 .. 2";
    if (const char *msg = parallax_rule(min_parallax_deg)) return msg;
    return q8_scale(scale);
}
// The scalars of lf_mkd_global_positions_device, of its host form and of its plan.
inline const char *positions_sweeps_rule(uint32_t sweeps) {
    return sweeps > LF_MKD_GLOBAL_POSITIONS_MAX_SWEEPS ? "sweeps must be 0 .. 4096 (each is three launches)" : nullptr;
}
inline const char *positions_scalars(uint32_t sweeps, float robust_deg, uint32_t min_obs, uint32_t flags) {
    if (flags) return "unknown flag bits (no flag is defined: flags must be 0)";
    if (const char *msg = positions_sweeps_rule(sweeps)) return msg;
    if (!(robust_deg > 0.f && robust_deg <= 90.f)) return "robust_deg must be in (0, 90]";
    if (min_obs < 2) return "min_obs must be at least 2";
    return nullptr;
}

// The sizes of a flat 8-bit call (and of its plan): the match needs a second candidate for its ratio test (min_candidates 2),
// the top-k and the grouped match answer from one.
inline const char *q8_sizes(uint64_t na, uint64_t nb, unsigned min_candidates) {
    if (nb < min_candidates) return min_candidates == 2 ? "needs at least two candidates in b" : "needs at least one candidate in b";
    if (above(kRowMax, na, nb)) return "more than 2^31 - 1 rows on a side";
    return nullptr;
}
// The arguments of a flat 8-bit call, device or host form.  any_null: one of the arrays it cannot do without is null;
// between: the call's own rule (nullptr: none, or met), which comes after the pointers and before the sizes.
inline const char *q8_args(const lf_mkd *h, bool any_null, const void *a, uint64_t na, const void *b, uint64_t nb, const void *lo,
                           const void *hi, bool device, unsigned min_candidates, const char *between = nullptr) {
    if (na && any_null) return "null pointer";
    if ((lo == nullptr) != (hi == nullptr)) return "exclude_lo and exclude_hi go together";
    if (device && na && misaligned(15, a, b)) return "d_a and d_b must be 16-byte aligned";
    if (between) return between;
    if (const char *msg = q8_sizes(na, nb, min_candidates)) return msg;
    return h ? nullptr : "null handle";
}

// A batch of pairs (or of edges over capacities): the rows of a side, and the grid `slots` gives one direction.
typedef uint64_t (*PairSlots)(uint64_t n_total, unsigned n_pairs);
inline const char *pairs_sizes(uint64_t na_total, uint64_t nb_total, uint32_t n_pairs, bool both, PairSlots slots, const char *too_many) {
    if (above(kRowMax, na_total, nb_total)) return "more than 2^31 - 1 rows on a side";
    if (slots(na_total, n_pairs) + (both ? slots(nb_total, n_pairs) : 0) > kRowMax) return too_many;
    return nullptr;
}
// The arguments of a batched matcher, in two calls: the arrays and the flags ...
inline const char *pairs_flags(bool any_null, uint32_t flags, const void *d_match_ba) {
    if (any_null) return "null pointer";
    if (flags & ~LF_MKD_MATCH_MUTUAL) return "unknown flag bits";
    if ((flags & LF_MKD_MATCH_MUTUAL) && !d_match_ba) return "LF_MKD_MATCH_MUTUAL needs d_match_ba";
    return nullptr;
}
// ... (a guided matcher's model in between) ...
inline const char *guide_rule(uint32_t kind, float threshold_px) {
    if (kind > LF_MKD_GUIDE_FUNDAMENTAL) return "kind must be LF_MKD_GUIDE_HOMOGRAPHY or LF_MKD_GUIDE_FUNDAMENTAL";
    return threshold_rule(threshold_px);
}
// ... then the rows, the grid and the handle.
inline const char *pairs_rows(const lf_mkd *h, const void *d_a, const void *d_b, uint64_t na_total, uint64_t nb_total, uint32_t n_pairs,
                              bool both, PairSlots slots, const char *too_many) {
    if (misaligned(15, d_a, d_b)) return "d_a and d_b must be 16-byte aligned";
    if (const char *msg = pairs_sizes(na_total, nb_total, n_pairs, both, slots, too_many)) return msg;
    return h ? nullptr : "null handle";
}

// ---- the host forms' staging ----------------------------------------------------------------------------------------------------
// One of the handle's byte arrays laid out as parts, each max(bytes, 1) rounded up to 16 (so every part is 16-byte aligned and
// empty parts do not share an address), with the copies to and from them on the handle's stream.  Declare the parts, reserve(),
// then copy; a Part is its array's address from then on.
template <typename T>
struct Part {
    unsigned char *const *base;
    uint64_t offset;
    T *get() const { return reinterpret_cast<T *>(*base + offset); }
    operator T *() const { return get(); }
};

struct Stager {
    lf_mkd *h;
    HipArray<unsigned char> &buf;
    unsigned char *base = nullptr;
    uint64_t total = 0;
    Stager(lf_mkd *h_, HipArray<unsigned char> &buf_) : h(h_), buf(buf_) {}
    Stager(const Stager &) = delete;
    template <typename T>
    Part<T> part(uint64_t count) {
        const Part<T> p{&base, total};
        total += (std::max<uint64_t>(count * sizeof(T), 1) + 15) / 16 * 16;
        return p;
    }
    int reserve() {
        if (int rc = grow(h, buf, total)) return rc;
        base = buf.get();
        return LF_MKD_OK;
    }
    // count elements to / from any device array, on the handle's stream; nothing for none
    template <typename T>
    hipError_t up(T *dst, const T *src, uint64_t count) const {
        return count ? hipMemcpyAsync(dst, src, count * sizeof(T), hipMemcpyHostToDevice, h->stream) : hipSuccess;
    }
    template <typename T>
    hipError_t down(T *dst, const T *src, uint64_t count) const {
        return count ? hipMemcpyAsync(dst, src, count * sizeof(T), hipMemcpyDeviceToHost, h->stream) : hipSuccess;
    }
    template <typename T>
    hipError_t up(Part<T> dst, const T *src, uint64_t count) const { return up(dst.get(), src, count); }
    template <typename T>
    hipError_t down(T *dst, Part<T> src, uint64_t count) const { return down(dst, static_cast<const T *>(src.get()), count); }
};

}  // namespace lfmkd
