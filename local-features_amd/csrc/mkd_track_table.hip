// gfx950 track tables (include/lf_mkd.h, lf_mkd_track_table_device / lf_mkd_gather_track_rows_device): the CSR
// table of the tracks lf_mkd_build_tracks_device labelled -- per kept track the ascending list of its rows -- made on the
// device in a fixed number of launches, and the row gather that brings the keypoints along.
//
//   tt_select        per block of kBlockRows rows: the number of selected roots and the 64-bit sum of their lengths;
//   tt_scan_blocks   one workgroup: the exclusive prefix of both over the blocks, the totals, d_counts;
//   tt_apply         per block: every selected root's table index i and W_i, the kept test, d_track_offsets[i], the
//                    label -> index map (scratch), and -- by the one root that is the first not kept -- T and O;
//   tt_keys          per row: key = the table index of its label (rows of no kept track: a key above every index, so they sort
//                    behind O), d_row_track, and the tail of d_track_offsets;
//   per radix pass   tt_hist (per block digit counts, [digit][block]), tt_scan_hist (one workgroup per digit: its exclusive
//                    prefix over the blocks, and its total), tt_scatter (stable: a row's rank among the rows of its digit
//                    is its rank in row order);
//   tt_finalise      d_obs_row and d_obs_image from the sorted rows in front of O.
//
// DETERMINISM.  A position is never decided by an atomic: the only atomics are the integer adds of tt_hist's LDS histogram,
// whose sums do not depend on their order.  Every scan is an exact integer prefix sum in a fixed order, every rank is a count
// of rows in front in row order, and launch boundaries are the only ordering between workgroups -- nobody waits, nothing
// assumes residency.  An LSD radix sort with stable passes sorts by (key, row): that is the table.
//
// COST IS DATA-INDEPENDENT.  Every launch touches every row once whatever the labels are; one track of all rows (every key
// equal, every row of a block in one digit) takes the same path as tracks of three rows.
//
// WHATEVER THE ARRAYS HOLD.  Indices read from the caller's arrays are checked against n before use; offsets are written at
// i < track_capacity (+ the tail up to track_capacity), rows at p < O <= obs_capacity.  W does not decrease whatever the
// lengths are (sums of uint32 in 64 bits, n < 2^31), so "kept" is a prefix and exactly one root is the first not kept.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/lf_mkd.h"
#include "mkd_block_scan.h"
#include "mkd_device.h"
#include "mkd_match_small.h"        // pair_rows, last_pair_at_or_before

#ifndef LF_MKD_TT_DIGIT_BITS
#define LF_MKD_TT_DIGIT_BITS 8      // the widest digit; chosen by measurement beside 6, 7, 9 and 11
#endif
#ifndef LF_MKD_TT_BLOCK_ROWS
#define LF_MKD_TT_BLOCK_ROWS 1024   // chosen by measurement beside 512, 2048 and 4096
#endif

namespace lfmkd {
namespace {

constexpr int kThreads = 256;                                 // every per-block kernel: 4 waves
constexpr int kWaves = kThreads / 64;
constexpr int kDigitBits = LF_MKD_TT_DIGIT_BITS;              // a pass sorts by at most this many bits: the key's bits are
constexpr int kRadix = 1 << kDigitBits;                       // spread evenly over the passes (20 bits: 7 + 7 + 6, not 8 + 8 + 4)
constexpr int kBlockRows = LF_MKD_TT_BLOCK_ROWS;              // rows one workgroup selects, counts and scatters
constexpr int kPer = kBlockRows / kThreads;                   // rows a thread; a wave owns kPer * 64 consecutive rows
constexpr int kScanThreads = 1024;                            // tt_scan_blocks, the one single-workgroup scan
constexpr int kGatherRows = 64;                               // rows one workgroup of gather_track_rows copies
static_assert(kBlockRows % kThreads == 0 && kPer >= 1 && kPer <= 32, "a thread owns kPer rows");
static_assert(kDigitBits >= 1 && kDigitBits <= 11, "kWaves * kRadix counters live in LDS");

__device__ __forceinline__ bool selected_root(const int *__restrict__ track, const unsigned *__restrict__ len,
                                              const unsigned *__restrict__ dup, long r, unsigned min_len, unsigned &l) {
    l = 0;
    if (track[r] != (int)r) return false;
    l = len[r];
    return l >= min_len && !(dup && dup[r] != 0u);            // (dup is null without LF_MKD_TRACK_TABLE_CONSISTENT)
}

}  // namespace

// n == 0: no track; the counts and every offset are 0
__global__ __launch_bounds__(kThreads) void tt_empty(uint64_t *__restrict__ offsets, long track_capacity,
                                                     unsigned *__restrict__ counts) {
    const long g = (long)blockIdx.x * kThreads + threadIdx.x;
    if (g < 4) counts[g] = 0u;
    if (g <= track_capacity) offsets[g] = 0ull;
}

__global__ __launch_bounds__(kThreads) void tt_select(const int *__restrict__ track, const unsigned *__restrict__ len,
                                                      const unsigned *__restrict__ dup, long n, unsigned min_len,
                                                      uint64_t *__restrict__ blk_len, unsigned *__restrict__ blk_cnt) {
    __shared__ uint64_t s_scan[2 * kThreads];
    const long r0 = (long)blockIdx.x * kBlockRows;
    unsigned cnt = 0;
    uint64_t sum = 0;
#pragma unroll
    for (int i = 0; i < kPer; ++i) {
        const long r = r0 + i * kThreads + threadIdx.x;
        unsigned l;
        if (r < n && selected_root(track, len, dup, r, min_len, l)) {
            ++cnt;
            sum += l;
        }
    }
    uint64_t total_cnt, total_len;
    block_scan<uint64_t, kThreads>(cnt, s_scan, total_cnt);
    block_scan<uint64_t, kThreads>(sum, s_scan, total_len);
    if (threadIdx.x == 0) {
        blk_cnt[blockIdx.x] = (unsigned)total_cnt;
        blk_len[blockIdx.x] = total_len;
    }
}

// One workgroup.  blk_cnt / blk_len [n_blocks] become their exclusive prefixes; counts[2], counts[3] are the wanted totals;
// counts[0], counts[1] are T and O if no capacity cuts anything, and otherwise 0 until tt_apply's one writer stores them.
__global__ __launch_bounds__(kScanThreads) void tt_scan_blocks(uint64_t *__restrict__ blk_len, unsigned *__restrict__ blk_cnt,
                                                               long n_blocks, uint64_t track_capacity, uint64_t obs_capacity,
                                                               unsigned *__restrict__ counts) {
    __shared__ uint64_t s_scan[2 * kScanThreads];
    const long per = (n_blocks + kScanThreads - 1) / kScanThreads;
    const long b0 = (long)threadIdx.x * per, b1 = b0 + per < n_blocks ? b0 + per : n_blocks;
    uint64_t cnt = 0, sum = 0;
    for (long b = b0; b < b1; ++b) {
        cnt += blk_cnt[b];
        sum += blk_len[b];
    }
    uint64_t total_cnt, total_len;
    cnt = block_scan<uint64_t, kScanThreads>(cnt, s_scan, total_cnt);
    sum = block_scan<uint64_t, kScanThreads>(sum, s_scan, total_len);
    for (long b = b0; b < b1; ++b) {
        const unsigned c = blk_cnt[b];
        const uint64_t l = blk_len[b];
        blk_cnt[b] = (unsigned)cnt;
        blk_len[b] = sum;
        cnt += c;
        sum += l;
    }
    if (threadIdx.x == 0) {
        const bool all = total_cnt <= track_capacity && total_len <= obs_capacity;
        counts[0] = all ? (unsigned)total_cnt : 0u;
        counts[1] = all ? (unsigned)total_len : 0u;
        counts[2] = (unsigned)total_cnt;
        counts[3] = total_len < 0xFFFFFFFFull ? (unsigned)total_len : 0xFFFFFFFFu;
    }
}

// Thread t owns rows [r0 + t kPer, r0 + (t + 1) kPer), so the scan over the threads is the scan over the rows.
__global__ __launch_bounds__(kThreads) void tt_apply(const int *__restrict__ track, const unsigned *__restrict__ len,
                                                     const unsigned *__restrict__ dup, long n, unsigned min_len,
                                                     const uint64_t *__restrict__ blk_len, const unsigned *__restrict__ blk_cnt,
                                                     uint64_t track_capacity, uint64_t obs_capacity,
                                                     uint64_t *__restrict__ offsets, int *__restrict__ map,
                                                     unsigned *__restrict__ counts) {
    __shared__ uint64_t s_scan[2 * kThreads];
    const long r0 = (long)blockIdx.x * kBlockRows + (long)threadIdx.x * kPer;
    unsigned l[kPer];
    unsigned sel = 0;                                         // bit i: row r0 + i is a selected root (kPer <= 32)
    uint64_t cnt = 0, sum = 0;
#pragma unroll
    for (int i = 0; i < kPer; ++i) {
        l[i] = 0;
        if (r0 + i < n && selected_root(track, len, dup, r0 + i, min_len, l[i])) {
            sel |= 1u << i;
            ++cnt;
            sum += l[i];
        }
    }
    uint64_t total;
    uint64_t idx = block_scan<uint64_t, kThreads>(cnt, s_scan, total) + blk_cnt[blockIdx.x];
    uint64_t w = block_scan<uint64_t, kThreads>(sum, s_scan, total) + blk_len[blockIdx.x];
#pragma unroll
    for (int i = 0; i < kPer; ++i) {
        if (r0 + i >= n) break;
        int at = -1;
        if (sel >> i & 1u) {
            const bool kept = idx < track_capacity && w + l[i] <= obs_capacity;
            if (kept) {
                offsets[idx] = w;
                at = (int)idx;                                // idx < track_capacity <= 2^31 - 1
            } else if (idx == 0 || (idx <= track_capacity && w <= obs_capacity)) {
                counts[0] = (unsigned)idx;                    // the track in front was kept, this one is not: T and O
                counts[1] = (unsigned)w;                      // (w <= obs_capacity, or idx == 0 and w == 0)
            }
            ++idx;
            w += l[i];
        }
        map[r0 + i] = at;
    }
}

// g < n: the row's key and d_row_track.  T < g <= track_capacity, and g == T: the tail of the offsets, O.
__global__ __launch_bounds__(kThreads) void tt_keys(const int *__restrict__ track, long n, const int *__restrict__ map,
                                                    unsigned key_none, long track_capacity,
                                                    const unsigned *__restrict__ counts, uint64_t *__restrict__ offsets,
                                                    unsigned *__restrict__ keys, int *__restrict__ row_track) {
    const long g = (long)blockIdx.x * kThreads + threadIdx.x;
    if (g < n) {
        const int t = track[g];
        const int at = t >= 0 && t < n ? map[t] : -1;
        if (row_track) row_track[g] = at;
        keys[g] = at >= 0 && (unsigned)at < key_none ? (unsigned)at : key_none;
    }
    if (g <= track_capacity && g >= (long)counts[0]) offsets[g] = counts[1];
}

__global__ __launch_bounds__(kThreads) void tt_hist(const unsigned *__restrict__ keys, long n, int shift, int bits, long n_blocks,
                                                    unsigned *__restrict__ hist) {
    __shared__ unsigned s_hist[kRadix];
    const int radix = 1 << bits;                              // (bits <= kDigitBits)
    for (int d = threadIdx.x; d < radix; d += kThreads) s_hist[d] = 0u;
    __syncthreads();
    const long r0 = (long)blockIdx.x * kBlockRows;
#pragma unroll
    for (int i = 0; i < kPer; ++i) {
        const long r = r0 + i * kThreads + threadIdx.x;
        if (r < n) atomicAdd(&s_hist[keys[r] >> shift & (radix - 1)], 1u);   // a sum: its order does not matter
    }
    __syncthreads();
    for (int d = threadIdx.x; d < radix; d += kThreads) hist[(long)d * n_blocks + blockIdx.x] = s_hist[d];
}

// One workgroup per digit: the digit's row hist[d][0 .. n_blocks) becomes its exclusive prefix over the blocks, and totals[d]
// the digit's count over all rows (the sums stay below n < 2^31).  The prefix over the DIGITS is tt_scatter's: it is the
// same kRadix numbers for every block, and a workgroup scans them in LDS faster than a launch could hand them over.
__global__ __launch_bounds__(kThreads) void tt_scan_hist(unsigned *__restrict__ hist, long n_blocks, unsigned *__restrict__ totals) {
    __shared__ unsigned s_scan[2 * kThreads];
    unsigned *row = hist + (long)blockIdx.x * n_blocks;
    const long per = (n_blocks + kThreads - 1) / kThreads;
    const long e0 = (long)threadIdx.x * per < n_blocks ? (long)threadIdx.x * per : n_blocks;
    const long e1 = e0 + per < n_blocks ? e0 + per : n_blocks;
    unsigned sum = 0;
    for (long e = e0; e < e1; ++e) sum += row[e];
    unsigned total;
    sum = block_scan<unsigned, kThreads>(sum, s_scan, total);
    for (long e = e0; e < e1; ++e) {
        const unsigned c = row[e];
        row[e] = sum;
        sum += c;
    }
    if (threadIdx.x == 0) totals[blockIdx.x] = total;
}

// The stable scatter of one pass.  Wave w owns rows [r0 + w kPer 64, r0 + (w + 1) kPer 64) and takes them 64 at a time, in
// order.  A round finds, per lane, the lanes of the wave with the same digit (one ballot per bit of the digit); a row's rank within its
// wave is the wave's running count of the digit (LDS, one counter per wave and digit) plus the lanes with it in front, and the
// lowest lane of every digit adds the round's count to the counter.  Then the counters turn into the first position of
// (digit, wave): the rows of all smaller digits (the prefix of totals, scanned here), plus the digit's rows in the blocks in
// front (tt_scan_hist), plus the counts of the waves in front.  vals_in null: the rows themselves (pass 0).  keys_out null: the
// last pass, whose keys nobody reads.
__global__ __launch_bounds__(kThreads) void tt_scatter(const unsigned *__restrict__ keys_in, const unsigned *__restrict__ vals_in,
                                                       long n, int shift, int bits, long n_blocks,
                                                       const unsigned *__restrict__ hist, const unsigned *__restrict__ totals, unsigned *__restrict__ keys_out,
                                                       unsigned *__restrict__ vals_out) {
    __shared__ unsigned s_cnt[kWaves * kRadix];
    __shared__ unsigned s_scan[2 * kThreads];
    const int radix = 1 << bits;                              // (bits <= kDigitBits)
    for (int d = threadIdx.x; d < kWaves * radix; d += kThreads) s_cnt[d] = 0u;
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long below = (1ull << lane) - 1ull;
    const long w0 = (long)blockIdx.x * kBlockRows + (long)wave * (kPer * 64) + lane;
    unsigned *mine = s_cnt + wave * radix;
    unsigned key[kPer], rank[kPer];
#pragma unroll
    for (int i = 0; i < kPer; ++i) {
        const long r = w0 + i * 64;
        const bool on = r < n;
        key[i] = on ? keys_in[r] : 0u;
        const unsigned d = key[i] >> shift & (radix - 1);
        unsigned long long peers = __ballot(on);
#pragma unroll
        for (int b = 0; b < kDigitBits; ++b) {
            if (b >= bits) break;                             // (uniform)
            const bool bit = d >> b & 1u;
            const unsigned long long vote = __ballot(bit);
            peers &= bit ? vote : ~vote;
        }
        const unsigned front = (unsigned)__popcll(peers & below);
        const unsigned base = on ? mine[d] : 0u;
        rank[i] = base + front;
        if (on && front == 0) mine[d] = base + (unsigned)__popcll(peers);
        __syncthreads();                                      // (uniform: every thread takes every round)
    }
    {                                                         // thread t: digits [t kPerDigit, (t + 1) kPerDigit)
        constexpr int kPerDigit = (kRadix + kThreads - 1) / kThreads;
        unsigned tot[kPerDigit], sum = 0, total;
#pragma unroll
        for (int i = 0; i < kPerDigit; ++i) {
            const int d = threadIdx.x * kPerDigit + i;
            tot[i] = d < radix ? totals[d] : 0u;
            sum += tot[i];
        }
        unsigned smaller = block_scan<unsigned, kThreads>(sum, s_scan, total);   // (its barriers also end the rounds above)
#pragma unroll
        for (int i = 0; i < kPerDigit; ++i) {
            const int d = threadIdx.x * kPerDigit + i;
            if (d < radix) {
                unsigned at = smaller + hist[(long)d * n_blocks + blockIdx.x];
#pragma unroll
                for (int w = 0; w < kWaves; ++w) {
                    const unsigned c = s_cnt[w * radix + d];
                    s_cnt[w * radix + d] = at;
                    at += c;
                }
            }
            smaller += tot[i];
        }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < kPer; ++i) {
        const long r = w0 + i * 64;
        if (r >= n) continue;
        const long at = (long)mine[key[i] >> shift & (radix - 1)] + rank[i];
        if (at >= n) continue;                                // (cannot happen: the counts are those of these very keys)
        if (keys_out) keys_out[at] = key[i];
        vals_out[at] = vals_in ? vals_in[r] : (unsigned)r;
    }
}

// the image whose range, read against the total as lf_mkd_build_tracks_device reads it, holds `row`; 0xFFFFFFFF: none
__device__ __forceinline__ unsigned image_of(const uint64_t *__restrict__ image_off, unsigned n_images, uint64_t total, long row) {
    if (n_images == 0) return 0xFFFFFFFFu;
    auto start = [&](unsigned m) { return image_off[m] < total ? image_off[m] : total; };
    const unsigned m = last_pair_at_or_before(n_images, (uint64_t)row, start);
    long lo, cnt;
    pair_rows(image_off[m], image_off[m + 1], total, lo, cnt);
    return row >= lo && row < lo + cnt ? m : 0xFFFFFFFFu;
}

__global__ __launch_bounds__(kThreads) void tt_finalise(const unsigned *__restrict__ rows, long n, long obs_capacity,
                                                        const unsigned *__restrict__ counts,
                                                        const uint64_t *__restrict__ image_off, unsigned n_images,
                                                        int *__restrict__ obs_row, unsigned *__restrict__ obs_image) {
    const long p = (long)blockIdx.x * kThreads + threadIdx.x;
    if (p >= n || p >= obs_capacity || p >= (long)counts[1]) return;
    const unsigned r = rows[p];
    obs_row[p] = (int)r;
    if (obs_image) obs_image[p] = image_of(image_off, n_images, (uint64_t)n, (long)r);
}

// dst row k = src row obs_row[k] for k < min(counts[1], obs_capacity); an index outside [0, n) gives a zero row
__global__ __launch_bounds__(kThreads) void gather_track_rows(const unsigned *__restrict__ src, unsigned row_words, long n,
                                                              const int *__restrict__ obs_row,
                                                              const unsigned *__restrict__ counts, long obs_capacity,
                                                              unsigned *__restrict__ dst) {
    const long count = (long)counts[1] < obs_capacity ? (long)counts[1] : obs_capacity;
    const long k0 = (long)blockIdx.x * kGatherRows;
    if (k0 >= count) return;
    const long k1 = k0 + kGatherRows < count ? k0 + kGatherRows : count;
    const int words = (int)(k1 - k0) * (int)row_words;
    for (int w = threadIdx.x; w < words; w += kThreads) {
        const long k = k0 + w / (int)row_words;
        const int c = w % (int)row_words;
        const int r = obs_row[k];
        dst[k * row_words + c] = r >= 0 && r < n ? src[(long)r * row_words + c] : 0u;
    }
}

TrackTablePlan track_table_plan(uint64_t n, unsigned min_len) {
    TrackTablePlan p{};
    const uint64_t bound = n / min_len;                       // no more tracks than this can be selected
    p.key_none = (unsigned)bound;
    for (uint64_t v = bound; v; v >>= 1) ++p.key_bits;
    p.passes = (p.key_bits + kDigitBits - 1) / kDigitBits;
    p.block_rows = kBlockRows;
    p.n_blocks = (n + kBlockRows - 1) / kBlockRows;
    if (n == 0) return p;
    // blk_len [n_blocks] u64 | map [n] | keys 0, 1 [n] | rows 0, 1 [n] | blk_cnt [n_blocks] | hist [radix][n_blocks] | totals [radix]
    p.off_map = p.n_blocks * 8;
    p.off_keys[0] = p.off_map + n * 4;
    p.off_keys[1] = p.off_keys[0] + n * 4;
    p.off_rows[0] = p.off_keys[1] + n * 4;
    p.off_rows[1] = p.off_rows[0] + n * 4;
    p.off_blk_cnt = p.off_rows[1] + n * 4;
    p.off_hist = p.off_blk_cnt + p.n_blocks * 4;
    p.off_totals = p.off_hist + (uint64_t)kRadix * p.n_blocks * 4;
    p.scratch_bytes = p.off_totals + (uint64_t)kRadix * 4;
    return p;
}

void launch_track_table(const TrackTablePlan &p, unsigned char *scratch, const uint64_t *image_off, unsigned n_images,
                        uint64_t total, const int *track, const unsigned *len, const unsigned *dup, unsigned min_len,
                        uint64_t track_capacity, uint64_t obs_capacity, uint64_t *offsets, int *obs_row, unsigned *obs_image,
                        int *row_track, unsigned *counts, hipStream_t stream) {
    const auto blocks = [](uint64_t items) { return dim3((unsigned)((items + kThreads - 1) / kThreads)); };
    if (total == 0) {
        hipLaunchKernelGGL(tt_empty, blocks(track_capacity + 1 > 4 ? track_capacity + 1 : 4), dim3(kThreads), 0, stream, offsets,
                           (long)track_capacity, counts);
        return;
    }
    const long n = (long)total, nb = (long)p.n_blocks;
    uint64_t *blk_len = reinterpret_cast<uint64_t *>(scratch);
    int *map = reinterpret_cast<int *>(scratch + p.off_map);
    unsigned *keys[2] = {reinterpret_cast<unsigned *>(scratch + p.off_keys[0]), reinterpret_cast<unsigned *>(scratch + p.off_keys[1])};
    unsigned *rows[2] = {reinterpret_cast<unsigned *>(scratch + p.off_rows[0]), reinterpret_cast<unsigned *>(scratch + p.off_rows[1])};
    unsigned *blk_cnt = reinterpret_cast<unsigned *>(scratch + p.off_blk_cnt);
    unsigned *hist = reinterpret_cast<unsigned *>(scratch + p.off_hist);
    unsigned *totals = reinterpret_cast<unsigned *>(scratch + p.off_totals);
    hipLaunchKernelGGL(tt_select, dim3((unsigned)nb), dim3(kThreads), 0, stream, track, len, dup, n, min_len, blk_len, blk_cnt);
    hipLaunchKernelGGL(tt_scan_blocks, dim3(1), dim3(kScanThreads), 0, stream, blk_len, blk_cnt, nb, track_capacity, obs_capacity,
                       counts);
    hipLaunchKernelGGL(tt_apply, dim3((unsigned)nb), dim3(kThreads), 0, stream, track, len, dup, n, min_len, blk_len, blk_cnt,
                       track_capacity, obs_capacity, offsets, map, counts);
    hipLaunchKernelGGL(tt_keys, blocks(total > track_capacity + 1 ? total : track_capacity + 1), dim3(kThreads), 0, stream, track,
                       n, map, p.key_none, (long)track_capacity, counts, offsets, keys[0], row_track);
    if (p.passes == 0 || obs_capacity == 0) return;           // no track can be kept: nothing in front of O
    int shift = 0;
    for (unsigned k = 0; k < p.passes; ++k) {
        const int bits = (int)(p.key_bits / p.passes + (k < p.key_bits % p.passes ? 1 : 0));   // evenly: all <= kDigitBits
        const bool last = k + 1 == p.passes;
        hipLaunchKernelGGL(tt_hist, dim3((unsigned)nb), dim3(kThreads), 0, stream, keys[k & 1], n, shift, bits, nb, hist);
        hipLaunchKernelGGL(tt_scan_hist, dim3(1u << bits), dim3(kThreads), 0, stream, hist, nb, totals);
        hipLaunchKernelGGL(tt_scatter, dim3((unsigned)nb), dim3(kThreads), 0, stream, keys[k & 1], k ? rows[k & 1] : nullptr, n,
                           shift, bits, nb, hist, totals, last ? nullptr : keys[(k + 1) & 1], rows[(k + 1) & 1]);
        shift += bits;
    }
    const uint64_t front = total < obs_capacity ? total : obs_capacity;
    hipLaunchKernelGGL(tt_finalise, blocks(front), dim3(kThreads), 0, stream, rows[p.passes & 1], n, (long)obs_capacity, counts,
                       image_off, n_images, obs_row, obs_image);
}

void launch_gather_track_rows(const void *src, unsigned row_bytes, uint64_t total, const int *obs_row, const unsigned *counts,
                              uint64_t obs_capacity, void *dst, hipStream_t stream) {
    if (obs_capacity == 0) return;
    hipLaunchKernelGGL(gather_track_rows, dim3((unsigned)((obs_capacity + kGatherRows - 1) / kGatherRows)), dim3(kThreads), 0,
                       stream, static_cast<const unsigned *>(src), row_bytes / 4, (long)total, obs_row, counts,
                       (long)obs_capacity, static_cast<unsigned *>(dst));
}

}  // namespace lfmkd
