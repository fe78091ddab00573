// C ABI, the matchers: f32 and 8-bit rows, flat, batched, guided and over edge lists; quantisation and the vote table.
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "lf_mkd_args.h"
#include "mkd_consts.hpp"

namespace {

constexpr uint64_t kMatchChunk = 1 << 20;   // a rows per pass of the two-pass matcher (2 GiB of records at one b split)

// the matcher's three words -- [0] largest |b| (float bits), [1] rows of the current chunk whose candidate records
// overflowed, [2] the same over the call (lf_mkd_match_overflowed) -- allocated on first use and zeroed once, on the stream
// the match will run on (so that a form that does not reset [2] adds to a defined value)
int ensure_match_misc(lf_mkd *h, hipStream_t s) {
    if (h->d_match_misc) return LF_MKD_OK;
    if (int rc = grow(h, h->d_match_misc, 3)) return rc;
    LF_HIP(h, hipMemsetAsync(h->d_match_misc, 0, 3 * sizeof(unsigned), s));
    return LF_MKD_OK;
}


// a flat call's plan, as the three plan calls report it
template <typename Plan>
int report_q8_plan(const Plan &p, uint32_t *a_blocks, uint32_t *b_splits, uint64_t *scratch_bytes) {
    if (a_blocks) *a_blocks = p.a_blocks;
    if (b_splits) *b_splits = p.splits;
    if (scratch_bytes) *scratch_bytes = p.scratch_bytes;
    return LF_MKD_OK;
}
int plan_cus(uint32_t num_cus) { return int(std::min<uint32_t>(num_cus, 1u << 20)); }

// The host forms stage a's rows, then b's (then what the call adds) in d_q8_io, and read the outputs out of d_match_out.
struct Q8Rows {
    Stager io;
    Part<uint8_t> a, b;
    Q8Rows(lf_mkd *h, uint64_t na, uint64_t nb) : io(h, h->d_q8_io), a(io.part<uint8_t>(na * kOut)), b(io.part<uint8_t>(nb * kOut)) {}
    hipError_t up(const uint8_t *rows_a, uint64_t na, const uint8_t *rows_b, uint64_t nb) const {
        const hipError_t e = io.up(a, rows_a, na * kOut);
        return e != hipSuccess ? e : io.up(b, rows_b, nb * kOut);
    }
};

}  // namespace

extern "C" {

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
    if (above(kRowMax, na, nb)) return fail(h, LF_MKD_ERR_BAD_ARG, "match: more than 2^31 rows");
    if (misaligned(15, d_a, d_b))
        return fail(h, LF_MKD_ERR_BAD_ARG, "match_device: d_a and d_b must be 16-byte aligned");
    LF_ENTER(h);
    hipStream_t s = stream_of(h, stream);
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
    return launched(h);
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
    if (misaligned(15, d_a, d_b))
        return fail(h, LF_MKD_ERR_BAD_ARG, "match_both_device: d_a and d_b must be 16-byte aligned");
    LF_ENTER(h);
    hipStream_t s = stream_of(h, stream);
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

// Many pairs in one call.  Like the verifiers it feeds, it checks its arguments before the handle (lf_mkd_args.h).
static const char kPairsGrid[] =
    "too many rows and pairs for one call (the grid needs floor(rows / 16) + n_pairs workgroups per direction, at most 2^31 - 1 in "
    "all)";

int lf_mkd_match_pairs_device(lf_mkd *h, const float *d_a, const uint64_t *d_offsets_a, uint64_t na_total, const float *d_b,
                              const uint64_t *d_offsets_b, uint64_t nb_total, uint32_t n_pairs, float ratio, uint32_t flags,
                              int32_t *d_match_ab, int32_t *d_match_ba, float *d_best, float *d_second, void *stream) {
    const char *msg = pairs_flags(!d_a || !d_b || !d_offsets_a || !d_offsets_b || !d_match_ab, flags, d_match_ba);
    if (!msg) msg = pairs_rows(h, d_a, d_b, na_total, nb_total, n_pairs, d_match_ba != nullptr, match_pairs_slots, kPairsGrid);
    if (msg) return refuse(h, "match_pairs_device", msg);
    if (n_pairs == 0) return LF_MKD_OK;
    LF_ENTER(h);
    launch_match_small_pairs(d_a, d_offsets_a, na_total, d_b, d_offsets_b, nb_total, n_pairs, ratio, (flags & LF_MKD_MATCH_MUTUAL) != 0,
                             d_match_ab, d_match_ba, d_best, d_second, h->d_match_misc ? h->d_match_misc + 2 : nullptr,
                             stream_of(h, stream));
    return launched(h);
}

// Guided matching: the same batch under each pair's verified model, its kind and threshold checked after the flags.
int lf_mkd_match_guided_pairs_device(lf_mkd *h, const float *d_a, const lf_mkd_keypoint *d_kps_a, const uint64_t *d_offsets_a,
                                     uint64_t na_total, const float *d_b, const lf_mkd_keypoint *d_kps_b,
                                     const uint64_t *d_offsets_b, uint64_t nb_total, const float *d_model, uint32_t n_pairs,
                                     uint32_t kind, float threshold_px, float ratio, uint32_t flags, int32_t *d_match_ab,
                                     int32_t *d_match_ba, float *d_best, float *d_second, void *stream) {
    const char *msg = pairs_flags(!d_a || !d_b || !d_kps_a || !d_kps_b || !d_offsets_a || !d_offsets_b || !d_model || !d_match_ab,
                                  flags, d_match_ba);
    if (!msg) msg = guide_rule(kind, threshold_px);
    if (!msg) msg = pairs_rows(h, d_a, d_b, na_total, nb_total, n_pairs, d_match_ba != nullptr, match_pairs_slots, kPairsGrid);
    if (msg) return refuse(h, "match_guided_pairs_device", msg);
    if (n_pairs == 0) return LF_MKD_OK;
    LF_ENTER(h);
    launch_match_guided_pairs(d_a, reinterpret_cast<const float *>(d_kps_a), d_offsets_a, na_total, d_b,
                              reinterpret_cast<const float *>(d_kps_b), d_offsets_b, nb_total, d_model, n_pairs, kind,
                              threshold_px, ratio, (flags & LF_MKD_MATCH_MUTUAL) != 0, d_match_ab, d_match_ba, d_best, d_second,
                              stream_of(h, stream));
    return launched(h);
}

int lf_mkd_match_overflowed(lf_mkd *h, void *stream, uint64_t *n_rows) {
    if (!h) return LF_MKD_ERR_BAD_ARG;
    if (!n_rows) return fail(h, LF_MKD_ERR_BAD_ARG, "match_overflowed: null pointer");
    *n_rows = 0;
    if (!h->d_match_misc) return LF_MKD_OK;           // no two-pass match yet
    LF_ENTER(h);
    hipStream_t s = stream_of(h, stream);
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
static const char *quantize_args(const lf_mkd *h, const void *desc, uint64_t n, float &scale, const void *q, bool device) {
    if (const char *msg = q8_scale(scale)) return msg;
    if (n && (!desc || !q)) return "null pointer";
    if (above(kRowMax, n)) return "more than 2^31 - 1 rows";
    if (device && n && (misaligned(15, desc) || misaligned(3, q))) return "d_desc must be 16-byte aligned and d_q 4-byte aligned";
    return h ? nullptr : "null handle";
}

int lf_mkd_quantize_descriptors_device(lf_mkd *h, const float *d_desc, uint64_t n, float scale, uint8_t *d_q, void *stream) {
    if (const char *msg = quantize_args(h, d_desc, n, scale, d_q, true)) return refuse(h, "quantize_descriptors_device", msg);
    if (n == 0) return LF_MKD_OK;
    LF_ENTER(h);
    launch_quantize_rows(d_desc, n, scale, d_q, stream_of(h, stream));
    return launched(h);
}

int lf_mkd_quantize_descriptors(lf_mkd *h, const float *desc, uint64_t n, float scale, uint8_t *q) {
    if (const char *msg = quantize_args(h, desc, n, scale, q, false)) return refuse(h, "quantize_descriptors", msg);
    if (n == 0) return LF_MKD_OK;
    LF_ENTER(h);
    if (int rc = grow(h, h->d_match_in, n * kOut)) return rc;
    Stager io(h, h->d_q8_io);
    const auto d_q = io.part<uint8_t>(n * kOut);
    if (int rc = io.reserve()) return rc;
    LF_HIP(h, io.up(h->d_match_in.get(), desc, n * kOut));
    launch_quantize_rows(h->d_match_in, n, scale, d_q, h->stream);
    LF_HIP(h, hipGetLastError());
    LF_HIP(h, io.down(q, d_q, n * kOut));
    LF_HIP(h, hipStreamSynchronize(h->stream));
    return LF_MKD_OK;
}

int lf_mkd_match_q8_plan(uint64_t na, uint64_t nb, uint32_t num_cus, uint32_t *a_blocks, uint32_t *b_splits,
                         uint64_t *scratch_bytes) {
    if (const char *msg = q8_sizes(na, nb, 2)) return refuse(nullptr, "match_q8_plan", msg);
    return report_q8_plan(match_q8_plan(long(na), long(nb), plan_cus(num_cus)), a_blocks, b_splits, scratch_bytes);
}

int lf_mkd_match_q8_device(lf_mkd *h, const uint8_t *d_a, uint64_t na, const uint8_t *d_b, uint64_t nb,
                           const uint32_t *d_exclude_lo, const uint32_t *d_exclude_hi, float ratio, int32_t *d_match,
                           int32_t *d_best, int32_t *d_second, void *stream) {
    if (const char *msg = q8_args(h, !d_a || !d_b || !d_match, d_a, na, d_b, nb, d_exclude_lo, d_exclude_hi, true, 2))
        return refuse(h, "match_q8_device", msg);
    if (na == 0) return LF_MKD_OK;
    LF_ENTER(h);
    const Q8Plan plan = match_q8_plan(long(na), long(nb), h->num_cus);
    unsigned char *partials;
    if (int rc = scratch(h, h->d_q8_part, plan.scratch_bytes, &partials)) return rc;
    launch_match_q8(d_a, long(na), d_b, long(nb), d_exclude_lo, d_exclude_hi, ratio, plan, partials, d_match, d_best, d_second,
                    stream_of(h, stream));
    return launched(h);
}

int lf_mkd_match_q8(lf_mkd *h, const uint8_t *a, uint64_t na, const uint8_t *b, uint64_t nb, float ratio, int32_t *match) {
    if (const char *msg = q8_args(h, !a || !b || !match, a, na, b, nb, nullptr, nullptr, false, 2)) return refuse(h, "match_q8", msg);
    if (na == 0) return LF_MKD_OK;
    LF_ENTER(h);
    Q8Rows rows(h, na, nb);
    if (int rc = rows.io.reserve()) return rc;
    if (int rc = grow(h, h->d_match_out, na)) return rc;
    LF_HIP(h, rows.up(a, na, b, nb));
    if (int rc = lf_mkd_match_q8_device(h, rows.a, na, rows.b, nb, nullptr, nullptr, ratio, h->d_match_out, nullptr, nullptr, h->stream))
        return rc;
    LF_HIP(h, rows.io.down(match, h->d_match_out.get(), na));
    LF_HIP(h, hipStreamSynchronize(h->stream));
    return LF_MKD_OK;
}

// The exact top-k over 8-bit rows (csrc/mkd_match_q8_knn.hip): the matcher's refusals, except that one candidate is an answer.
static const char *knn_rule(uint32_t k) { return k == 0 || k > LF_MKD_KNN_MAX ? "k must be 1 .. LF_MKD_KNN_MAX (16)" : nullptr; }

int lf_mkd_knn_q8_plan(uint64_t na, uint64_t nb, uint32_t k, uint32_t num_cus, uint32_t *a_blocks, uint32_t *b_splits,
                       uint64_t *scratch_bytes) {
    const char *msg = knn_rule(k);
    if (!msg) msg = q8_sizes(na, nb, 1);
    if (msg) return refuse(nullptr, "knn_q8_plan", msg);
    return report_q8_plan(knn_q8_plan(long(na), long(nb), int(k), plan_cus(num_cus)), a_blocks, b_splits, scratch_bytes);
}

int lf_mkd_knn_q8_device(lf_mkd *h, const uint8_t *d_a, uint64_t na, const uint8_t *d_b, uint64_t nb,
                         const uint32_t *d_exclude_lo, const uint32_t *d_exclude_hi, uint32_t k, int32_t *d_index,
                         int32_t *d_score, void *stream) {
    if (const char *msg = q8_args(h, !d_a || !d_b || !d_index, d_a, na, d_b, nb, d_exclude_lo, d_exclude_hi, true, 1, knn_rule(k)))
        return refuse(h, "knn_q8_device", msg);
    if (na == 0) return LF_MKD_OK;
    LF_ENTER(h);
    const KnnQ8Plan plan = knn_q8_plan(long(na), long(nb), int(k), h->num_cus);
    unsigned char *partials;
    if (int rc = scratch(h, h->d_q8_part, plan.scratch_bytes, &partials)) return rc;
    launch_knn_q8(d_a, long(na), d_b, long(nb), d_exclude_lo, d_exclude_hi, int(k), plan, partials, d_index, d_score,
                  stream_of(h, stream));
    return launched(h);
}

int lf_mkd_knn_q8(lf_mkd *h, const uint8_t *a, uint64_t na, const uint8_t *b, uint64_t nb, uint32_t k, int32_t *index,
                  int32_t *score) {
    if (const char *msg = q8_args(h, !a || !b || !index, a, na, b, nb, nullptr, nullptr, false, 1, knn_rule(k)))
        return refuse(h, "knn_q8", msg);
    if (na == 0) return LF_MKD_OK;
    LF_ENTER(h);
    Q8Rows rows(h, na, nb);
    if (int rc = rows.io.reserve()) return rc;
    if (int rc = grow(h, h->d_match_out, 2 * na * k)) return rc;
    int *d_index = h->d_match_out, *d_score = score ? d_index + na * k : nullptr;
    LF_HIP(h, rows.up(a, na, b, nb));
    if (int rc = lf_mkd_knn_q8_device(h, rows.a, na, rows.b, nb, nullptr, nullptr, k, d_index, d_score, h->stream)) return rc;
    LF_HIP(h, rows.io.down(index, d_index, na * k));
    LF_HIP(h, rows.io.down(score, d_score, score ? na * k : 0));
    LF_HIP(h, hipStreamSynchronize(h->stream));
    return LF_MKD_OK;
}

// Grouped matching over 8-bit rows (csrc/mkd_match_q8_grouped.hip): the matcher's refusals, except that one candidate is an
// answer; the rival is the best score of another group than the best's.
int lf_mkd_match_q8_grouped_plan(uint64_t na, uint64_t nb, uint32_t num_cus, uint32_t *a_blocks, uint32_t *b_splits,
                                 uint64_t *scratch_bytes) {
    if (const char *msg = q8_sizes(na, nb, 1)) return refuse(nullptr, "match_q8_grouped_plan", msg);
    return report_q8_plan(match_q8_grouped_plan(long(na), long(nb), plan_cus(num_cus)), a_blocks, b_splits, scratch_bytes);
}

int lf_mkd_match_q8_grouped_device(lf_mkd *h, const uint8_t *d_a, uint64_t na, const uint8_t *d_b, uint64_t nb,
                                   const uint32_t *d_group_of_b, const uint32_t *d_exclude_lo, const uint32_t *d_exclude_hi,
                                   float ratio, int32_t *d_match, int32_t *d_best, int32_t *d_rival, void *stream) {
    const char *words = na && misaligned(3, d_group_of_b, d_exclude_lo, d_exclude_hi, d_match, d_best, d_rival)
                            ? "d_group_of_b, the exclusion bounds and the outputs must be 4-byte aligned"
                            : nullptr;
    if (const char *msg = q8_args(h, !d_a || !d_b || !d_group_of_b || !d_match, d_a, na, d_b, nb, d_exclude_lo, d_exclude_hi, true, 1, words))
        return refuse(h, "match_q8_grouped_device", msg);
    if (na == 0) return LF_MKD_OK;
    LF_ENTER(h);
    const Q8GroupedPlan plan = match_q8_grouped_plan(long(na), long(nb), h->num_cus);
    unsigned char *partials;
    if (int rc = scratch(h, h->d_q8_part, plan.scratch_bytes, &partials)) return rc;
    launch_match_q8_grouped(d_a, long(na), d_b, long(nb), d_group_of_b, d_exclude_lo, d_exclude_hi, ratio, plan, partials, d_match,
                            d_best, d_rival, stream_of(h, stream));
    return launched(h);
}

int lf_mkd_match_q8_grouped(lf_mkd *h, const uint8_t *a, uint64_t na, const uint8_t *b, uint64_t nb,
                            const uint32_t *group_of_b, float ratio, int32_t *match, int32_t *best, int32_t *rival) {
    if (const char *msg = q8_args(h, !a || !b || !group_of_b || !match, a, na, b, nb, nullptr, nullptr, false, 1))
        return refuse(h, "match_q8_grouped", msg);
    if (na == 0) return LF_MKD_OK;
    LF_ENTER(h);
    Q8Rows rows(h, na, nb);   // ... and then b's group ids ((na + nb) * 128 keeps them 4-byte aligned)
    const auto d_group = rows.io.part<uint32_t>(nb);
    if (int rc = rows.io.reserve()) return rc;
    if (int rc = grow(h, h->d_match_out, 3 * na)) return rc;
    int *d_match = h->d_match_out, *d_best = best ? d_match + na : nullptr, *d_rival = rival ? d_match + 2 * na : nullptr;
    LF_HIP(h, rows.up(a, na, b, nb));
    LF_HIP(h, rows.io.up(d_group, group_of_b, nb));
    if (int rc = lf_mkd_match_q8_grouped_device(h, rows.a, na, rows.b, nb, d_group, nullptr, nullptr, ratio, d_match, d_best, d_rival,
                                                h->stream))
        return rc;
    LF_HIP(h, rows.io.down(match, d_match, na));
    LF_HIP(h, rows.io.down(best, d_best, best ? na : 0));
    LF_HIP(h, rows.io.down(rival, d_rival, rival ? na : 0));
    LF_HIP(h, hipStreamSynchronize(h->stream));
    return LF_MKD_OK;
}

// The group-by-group vote table of a match array: a zeroing launch and one launch of integer atomic adds.
int lf_mkd_vote_groups_device(lf_mkd *h, const int32_t *d_match, uint64_t na, const uint32_t *d_group_of_a, uint32_t n_groups_a,
                              const uint32_t *d_group_of_b, uint64_t nb, uint32_t n_groups_b, uint32_t *d_votes, void *stream) {
    const char *msg = nullptr;
    if (na && (!d_match || !d_group_of_b)) msg = "null pointer";
    else if (n_groups_a == 0 || n_groups_b == 0) msg = "a group count of zero";
    else if (above(kRowMax, uint64_t(n_groups_a) * n_groups_b)) msg = "more than 2^31 - 1 entries in the vote table";
    else if (!d_votes) msg = "null d_votes";
    else if (above(kRowMax, na, nb)) msg = "more than 2^31 - 1 rows on a side";
    else if (misaligned(3, d_match, d_group_of_a, d_group_of_b, d_votes)) msg = "the arrays must be 4-byte aligned";
    else if (!h) msg = "null handle";
    if (msg) return refuse(h, "vote_groups_device", msg);
    LF_ENTER(h);
    launch_vote_groups(d_match, long(na), d_group_of_a, n_groups_a, d_group_of_b, long(nb), n_groups_b, d_votes, stream_of(h, stream));
    return launched(h);
}

// Many pairs of 8-bit rows in one call: lf_mkd_match_pairs_device's layout and refusals, the int8 matcher's decisions.
static const char kQ8PairsGrid[] =
    "too many rows and pairs for one call (the grid needs floor(rows / block_rows) + n_pairs workgroups per direction, at most "
    "2^31 - 1 in all)";

int lf_mkd_match_q8_pairs_plan(uint64_t na_total, uint64_t nb_total, uint32_t n_pairs, uint32_t both_directions,
                               uint32_t *block_rows, uint64_t *workgroups) {
    if (const char *msg = pairs_sizes(na_total, nb_total, n_pairs, both_directions != 0, match_q8_pairs_slots, kQ8PairsGrid))
        return refuse(nullptr, "match_q8_pairs_plan", msg);
    if (block_rows) *block_rows = match_q8_pairs_block_rows();
    if (workgroups)
        *workgroups = match_q8_pairs_slots(na_total, n_pairs) + (both_directions ? match_q8_pairs_slots(nb_total, n_pairs) : 0);
    return LF_MKD_OK;
}

int lf_mkd_match_q8_pairs_device(lf_mkd *h, const uint8_t *d_a, const uint64_t *d_offsets_a, uint64_t na_total,
                                 const uint8_t *d_b, const uint64_t *d_offsets_b, uint64_t nb_total, uint32_t n_pairs,
                                 float ratio, uint32_t flags, int32_t *d_match_ab, int32_t *d_match_ba, int32_t *d_best,
                                 int32_t *d_second, void *stream) {
    const char *msg = pairs_flags(!d_a || !d_b || !d_offsets_a || !d_offsets_b || !d_match_ab, flags, d_match_ba);
    if (!msg) msg = pairs_rows(h, d_a, d_b, na_total, nb_total, n_pairs, d_match_ba != nullptr, match_q8_pairs_slots, kQ8PairsGrid);
    if (msg) return refuse(h, "match_q8_pairs_device", msg);
    if (n_pairs == 0) return LF_MKD_OK;
    LF_ENTER(h);
    launch_match_q8_pairs(d_a, d_offsets_a, na_total, d_b, d_offsets_b, nb_total, n_pairs, ratio, (flags & LF_MKD_MATCH_MUTUAL) != 0,
                          d_match_ab, d_match_ba, d_best, d_second, stream_of(h, stream));
    return launched(h);
}

// Guided matching over 8-bit rows: the two calls' refusals together, the q8 pairs call's grid.
int lf_mkd_match_q8_guided_pairs_device(lf_mkd *h, const uint8_t *d_a, const lf_mkd_keypoint *d_kps_a, const uint64_t *d_offsets_a,
                                        uint64_t na_total, const uint8_t *d_b, const lf_mkd_keypoint *d_kps_b,
                                        const uint64_t *d_offsets_b, uint64_t nb_total, const float *d_model, uint32_t n_pairs,
                                        uint32_t kind, float threshold_px, float ratio, uint32_t flags, int32_t *d_match_ab,
                                        int32_t *d_match_ba, int32_t *d_best, int32_t *d_second, void *stream) {
    const char *msg = pairs_flags(!d_a || !d_b || !d_kps_a || !d_kps_b || !d_offsets_a || !d_offsets_b || !d_model || !d_match_ab,
                                  flags, d_match_ba);
    if (!msg) msg = guide_rule(kind, threshold_px);
    if (!msg) msg = pairs_rows(h, d_a, d_b, na_total, nb_total, n_pairs, d_match_ba != nullptr, match_q8_pairs_slots, kQ8PairsGrid);
    if (msg) return refuse(h, "match_q8_guided_pairs_device", msg);
    if (n_pairs == 0) return LF_MKD_OK;
    LF_ENTER(h);
    launch_match_q8_guided_pairs(d_a, reinterpret_cast<const float *>(d_kps_a), d_offsets_a, na_total, d_b,
                                 reinterpret_cast<const float *>(d_kps_b), d_offsets_b, nb_total, d_model, n_pairs, kind,
                                 threshold_px, ratio, (flags & LF_MKD_MATCH_MUTUAL) != 0, d_match_ab, d_match_ba, d_best, d_second,
                                 stream_of(h, stream));
    return launched(h);
}

// Edge-list matching over 8-bit rows (csrc/mkd_match_q8_edges.hip): pools, edges and edge layouts.
int lf_mkd_edge_layout_device(lf_mkd *h, const uint64_t *d_image_offsets, uint32_t n_images, uint64_t n_rows_total,
                              const uint32_t *d_edge_image, uint32_t n_edges, uint64_t *d_edge_offsets, void *stream) {
    const char *msg = nullptr;
    if (n_edges && (!d_image_offsets || !d_edge_image || !d_edge_offsets)) msg = "null pointer";
    else if (misaligned(7, d_image_offsets, d_edge_offsets)) msg = "the offset arrays must be 8-byte aligned";
    else if (misaligned(3, d_edge_image)) msg = "d_edge_image must be 4-byte aligned";
    else if (above(kRowMax, n_rows_total)) msg = "more than 2^31 - 1 rows in the pool";
    else if (!h) msg = "null handle";
    if (msg) return refuse(h, "edge_layout_device", msg);
    if (n_edges == 0) return LF_MKD_OK;
    LF_ENTER(h);
    launch_edge_layout(d_image_offsets, n_images, n_rows_total, d_edge_image, n_edges, d_edge_offsets, stream_of(h, stream));
    return launched(h);
}

int lf_mkd_gather_edge_rows_device(lf_mkd *h, const void *d_src, uint32_t row_bytes, const uint64_t *d_image_offsets,
                                   uint32_t n_images, uint64_t n_rows_total, const uint32_t *d_edge_image,
                                   const uint64_t *d_edge_offsets, uint64_t capacity_rows, uint32_t n_edges, void *d_dst,
                                   void *stream) {
    const char *msg = nullptr;
    if (!d_src || !d_image_offsets || !d_edge_image || !d_edge_offsets || !d_dst) msg = "null pointer";
    else if (row_bytes < 4 || row_bytes > 512 || (row_bytes & 3)) msg = "row_bytes must be a multiple of 4 in [4, 512]";
    else if (misaligned(3, d_src, d_dst)) msg = "d_src and d_dst must be 4-byte aligned";
    else if (above(kRowMax, n_rows_total, capacity_rows)) msg = "a total or a capacity above 2^31 - 1 rows";
    else if (above(kRowMax, capacity_rows / gather_edge_rows_block_rows() + n_edges))
        msg = "too many rows and edges for one call (the grid needs floor(capacity / block_rows) + n_edges workgroups, at most 2^31 - 1)";
    else if (!h) msg = "null handle";
    if (msg) return refuse(h, "gather_edge_rows_device", msg);
    if (n_edges == 0) return LF_MKD_OK;
    LF_ENTER(h);
    launch_gather_edge_rows(d_src, row_bytes, d_image_offsets, n_images, n_rows_total, d_edge_image, d_edge_offsets, capacity_rows,
                            n_edges, d_dst, stream_of(h, stream));
    return launched(h);
}

int lf_mkd_match_q8_edges_device(lf_mkd *h, const uint8_t *d_a, const uint64_t *d_image_offsets_a, uint32_t n_images_a,
                                 uint64_t na_total, const uint8_t *d_b, const uint64_t *d_image_offsets_b, uint32_t n_images_b,
                                 uint64_t nb_total, const uint32_t *d_edge_a, const uint32_t *d_edge_b,
                                 const uint64_t *d_edge_offsets_a, uint64_t ea_capacity, const uint64_t *d_edge_offsets_b,
                                 uint64_t eb_capacity, uint32_t n_edges, float ratio, uint32_t flags, int32_t *d_match_ab,
                                 int32_t *d_match_ba, int32_t *d_best, int32_t *d_second, void *stream) {
    const char *msg = nullptr;
    if (!d_a || !d_b || !d_image_offsets_a || !d_image_offsets_b || !d_match_ab) msg = "null pointer";
    else if (!d_edge_a || !d_edge_b) msg = "null edge array";
    else if (!d_edge_offsets_a) msg = "null layout array";
    else if ((msg = pairs_flags(false, flags, d_match_ba))) {}
    else if (d_match_ba && !d_edge_offsets_b) msg = "null layout array: d_match_ba needs d_edge_offsets_b";
    else if (misaligned(15, d_a, d_b)) msg = "d_a and d_b must be 16-byte aligned";
    else if (above(kRowMax, na_total, nb_total, ea_capacity, eb_capacity)) msg = "a total or a capacity above 2^31 - 1 rows";
    // the grid is the pairs call's over the capacities: the same plan, the same words
    else if (!(msg = pairs_sizes(ea_capacity, eb_capacity, n_edges, d_match_ba != nullptr, match_q8_pairs_slots, kQ8PairsGrid)) && !h)
        msg = "null handle";
    if (msg) return refuse(h, "match_q8_edges_device", msg);
    if (n_edges == 0) return LF_MKD_OK;
    LF_ENTER(h);
    launch_match_q8_edges(d_a, d_image_offsets_a, n_images_a, na_total, d_b, d_image_offsets_b, n_images_b, nb_total, d_edge_a,
                          d_edge_b, d_edge_offsets_a, ea_capacity, d_edge_offsets_b, eb_capacity, n_edges, ratio,
                          (flags & LF_MKD_MATCH_MUTUAL) != 0, d_match_ab, d_match_ba, d_best, d_second, stream_of(h, stream));
    return launched(h);
}

}  // extern "C"
