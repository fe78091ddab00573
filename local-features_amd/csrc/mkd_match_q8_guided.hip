// gfx950 guided matching over 8-bit descriptors (lf_mkd_match_q8_guided_pairs_device, include/lf_mkd.h): the
// batched int8 matcher of mkd_match_q8.hip once more, with each row's candidates restricted to the rows of the other side
// that the pair's verified model allows -- mkd_match_guided.hip's admissibility relation over mkd_match_q8.hip's sums.
//
// `match_q8_guided_pairs` has match_q8_pairs' slot map, workgroup shape (R = kPRows rows of x per workgroup, one 32-row tile
// per wave), clamps to the pair and y stream: the per-lane LDS-DMA into the [chunk 8][row 32][16 B] tile image, kPStage tiles
// per stage, double buffered, vmcnt(0) plus a barrier per stage.  Every wave issues its DMA pieces and meets every barrier,
// whatever its votes: the stream is NOT made conditional here (a stage could only be skipped on a workgroup-wide vote taken
// ahead of its issue).  What is added sits IN FRONT of a 32 x 32 tile: lane (r, h) owns x row r of its wave's tile, keeps that
// row's share of the predicate in registers and tests it against its 16 y rows 32 t + 4 h + (i & 3) + 8 (i >> 2) -- the
// accumulator's layout --; a wave-wide vote then decides whether the tile is run at all.  A tile without an admissible pair
// costs no fragment read, no MFMA and no epilogue; in a tile that is run the inadmissible sums become INT32_MIN, below every
// sum, as the rows beyond the pair's end always were.
//
// The y side's keypoints travel with the y stream: threads 0 .. 127 request x and y of the next stage's 128 rows when they
// issue its DMA (a row beyond the pair's last is the pair's last), and write them to the other of two 2 KiB buffers at the end
// of the stage they were requested in, in front of the barrier that opens theirs.  What depends on the y row alone is
// computed there, once, instead of once per x row: the mapped point under a homography in the reverse direction, the epipolar
// line or the denominator's inner links under a fundamental matrix (mkd_guided_math.h's own hoisted forms: operations move,
// none is reordered or re-associated).
//
// The admissibility test is the verifiers' inlier test, op for op, with the model's nine floats in scalar registers; both
// directions evaluate pred(a_i, b_j).  Contraction: mkd_guided_math.h switches it off for the rest of this unit, which is why
// the kernel has a unit of its own; the similarity is integer MFMAs, to which the mode makes no difference.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>

#include "mkd_device.h"
#include "mkd_match_q8_batched.h"  // q8_pairs_slot, q8_issue_stage, q8_take_tile, q8_fold_halves, the kP* shape

#include "mkd_guided_math.h"   // (last: its file-scope pragma holds from here on)

namespace lfmkd {
namespace {

static_assert(kPTiles == 1, "a lane owns one x row: the guided form is written for one tile per wave");
constexpr int kGStageRows = kPStage * kQTileRows;   // y rows per stage: 128
static_assert(kPThreads >= kGStageRows, "one staging thread per y row of a stage");

// MODE = 2 kind + rev.  `stage`: what is kept of a y row's keypoint (qx, qy), 16 bytes; the constructor: what a lane keeps of
// its own x row; `test`: the one against the other.  Together each is guide_admissible() of mkd_guided_math.h.
template <int MODE>
struct GuideQ;
template <>
struct GuideQ<0> {   // homography, x = a: the mapped point is the x row's, a y row brings its coordinates
    GuideHA a;
    __device__ __forceinline__ GuideQ(const float *m, float px, float py, float thr2) : a(guide_h_of_a(m, px, py, thr2)) {}
    static __device__ __forceinline__ float4 stage(const float *, float qx, float qy, float) { return make_float4(qx, qy, 0.f, 0.f); }
    __device__ __forceinline__ bool test(const float4 &q, float) const { return guide_h_test(a, q.x, q.y); }
};
template <>
struct GuideQ<1> {   // homography, x = b: every y row is mapped, once
    float bx, by;
    __device__ __forceinline__ GuideQ(const float *, float px, float py, float) : bx(px), by(py) {}
    static __device__ __forceinline__ float4 stage(const float *m, float qx, float qy, float thr2) {
        const GuideHA g = guide_h_of_a(m, qx, qy, thr2);
        return make_float4(g.u, g.v, g.w, g.lim);
    }
    __device__ __forceinline__ bool test(const float4 &q, float) const {
        GuideHA g;
        g.u = q.x; g.v = q.y; g.w = q.z; g.lim = q.w;
        return guide_h_test(g, bx, by);
    }
};
template <>
struct GuideQ<2> {   // fundamental matrix, x = a: the x row's epipolar line; a y row brings F^T b's share of the denominator
    GuideFA a;
    __device__ __forceinline__ GuideQ(const float *m, float px, float py, float) : a(guide_f_of_a(m, px, py)) {}
    static __device__ __forceinline__ float4 stage(const float *m, float qx, float qy, float) {
        const GuideFB g = guide_f_of_b(m, qx, qy);
        return make_float4(g.bx, g.by, g.mm, 0.f);
    }
    __device__ __forceinline__ bool test(const float4 &q, float thr2) const {
        GuideFB g;
        g.bx = q.x; g.by = q.y; g.mm = q.z;
        return guide_f_test(a, g, thr2);
    }
};
template <>
struct GuideQ<3> {   // fundamental matrix, x = b: a y row brings its epipolar line
    GuideFB b;
    __device__ __forceinline__ GuideQ(const float *m, float px, float py, float) : b(guide_f_of_b(m, px, py)) {}
    static __device__ __forceinline__ float4 stage(const float *m, float qx, float qy, float) {
        const GuideFA g = guide_f_of_a(m, qx, qy);
        return make_float4(g.l0, g.l1, g.l2, 0.f);
    }
    __device__ __forceinline__ bool test(const float4 &q, float thr2) const {
        GuideFA g;
        g.l0 = q.x; g.l1 = q.y; g.l2 = q.z;
        return guide_f_test(g, b, thr2);
    }
};

struct Q8GuidedShared {
    unsigned char y[2][kPStage * kQTileBytes];   // the y stream's two stages: 32 KiB
    float4 kp[2][kGStageRows];                   // ... and their rows' staged keypoints: 4 KiB
};

// The body of a workgroup: q8_pairs_block's walk (mkd_match_q8_batched.h) over x [nx][128] against y [ny][128] with the vote in
// front of every tile.
// kx / ky: the two sides' keypoints (rows of 5 floats), m: the pair's model.  nx >= 1 and ny >= 1.
template <int MODE>
__device__ __forceinline__ void q8_guided_block(const unsigned char *__restrict__ x, const float *__restrict__ kx, long nx,
                                                const unsigned char *__restrict__ y, const float *__restrict__ ky, long ny,
                                                const float *__restrict__ m, float thr2, float ratio, int *__restrict__ match,
                                                int *__restrict__ best_o, int *__restrict__ second_o, long block,
                                                Q8GuidedShared &sh) {
    typedef GuideQ<MODE> G;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int r = lane & 31, h = lane >> 5;
    const long x_tile = block * kPWaves + wave;
    const long x_tiles_total = (nx + kQTileRows - 1) / kQTileRows;
    const long y_tiles_total = (ny + kQTileRows - 1) / kQTileRows;
    // a wave whose x tile does not exist skips every tile (wave-uniform; it still takes part in the DMA issues, the keypoint
    // staging and the barriers)
    const bool wave_live = x_tile < x_tiles_total;
    const long xrow = x_tile * kQTileRows + r;
    const bool x_live = wave_live && xrow < nx;
    const long xrow_c = xrow < nx ? xrow : nx - 1;                                       // idle rows redo the PAIR's last one
    // x fragments: B operand of the MFMA, lane (r, h) holds the bytes 32 s + 16 h .. + 15 of its row
    i32x4 xf[4];
    {
        const unsigned char *src = x + xrow_c * 128 + 16 * h;
#pragma unroll
        for (int s = 0; s < 4; ++s) xf[s] = *reinterpret_cast<const i32x4 *>(src + 32 * s) ^ kSignBits;
    }
    const G mine(m, kx[xrow_c * 5], kx[xrow_c * 5 + 1], thr2);
    int best = INT_MIN, second = INT_MIN, best_i = -1;

    // the keypoint of row threadIdx.x of a stage (a row beyond the pair's last: the pair's last, masked in the vote)
    const bool stager = threadIdx.x < kGStageRows;                                       // (whole waves)
    float qx = 0.f, qy = 0.f;
    auto request_kp = [&](long t) {
        long row = t * kQTileRows + (long)threadIdx.x;
        row = row < ny ? row : ny - 1;
        qx = ky[row * 5];
        qy = ky[row * 5 + 1];
    };
    q8_issue_stage(y, ny, 0, &sh.y[0][0], wave);
    if (stager) {
        request_kp(0);
        sh.kp[0][threadIdx.x] = G::stage(m, qx, qy, thr2);
    }
    for (long t0 = 0; t0 < y_tiles_total; t0 += kPStage) {
        const int buf = (int)((t0 / kPStage) & 1);
        __builtin_amdgcn_s_waitcnt(0x0f70);   // vmcnt(0): this wave's pieces of the stage have landed
        __syncthreads();                      // ... and everybody's, and its keypoints; everybody is done with the other buffers
        const bool more = t0 + kPStage < y_tiles_total;
        if (more) {
            q8_issue_stage(y, ny, t0 + kPStage, &sh.y[buf ^ 1][0], wave);
            if (stager) request_kp(t0 + kPStage);   // in flight beside the DMA while this stage is worked on
        }
#pragma unroll
        for (int u = 0; u < kPStage; ++u) {
            const long t = t0 + u;
            if (t >= y_tiles_total || !wave_live) break;
            const int row0 = (int)(t * kQTileRows) + 4 * h;
            // the vote: the lane's 16 bits of the tile.  A y row at or beyond ny and an x row at or beyond nx are never
            // admissible; the branch on the ballot is wave-uniform.
            const float4 *kq = &sh.kp[buf][u * kQTileRows + 4 * h];
            unsigned adm = 0u;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int o = (i & 3) + 8 * (i >> 2);
                const bool ok = mine.test(kq[o], thr2) && row0 + o < ny && x_live;
                adm |= ok ? 1u << i : 0u;
            }
            if (__builtin_amdgcn_ballot_w64(adm != 0u) == 0ull) continue;   // no fragment read, no MFMA, no epilogue
            const unsigned char *yy = &sh.y[buf][0] + u * kQTileBytes + (h * 32 + r) * 16;
            i32x4 yf[4];
#pragma unroll
            for (int s = 0; s < 4; ++s) yf[s] = *reinterpret_cast<const i32x4 *>(yy + s * 1024) ^ kSignBits;
            i32x16 acc;
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[i] = 0;
#pragma unroll
            for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(yf[s], xf[s], acc, 0, 0, 0);
#pragma unroll
            for (int i = 0; i < 16; ++i)      // inadmissible pairs, the rows beyond the pair's last y row among them
                if (!((adm >> i) & 1u)) acc[i] = INT_MIN;
            q8_take_tile(acc, row0, best, second, best_i);
        }
        // the next stage's keypoints -> the other buffer, whose readers all passed this stage's barrier
        if (more && stager) sh.kp[buf ^ 1][threadIdx.x] = G::stage(m, qx, qy, thr2);
    }
    const Q8Top top = q8_fold_halves(best, second, best_i);
    const int nbest = top.best, nsecond = top.second, nidx = top.index;
    if (h == 0 && x_live) {
        match[xrow] = q8_decide(nbest, nidx, nsecond, ratio);
        if (best_o) best_o[xrow] = nbest;
        if (second_o) second_o[xrow] = nsecond;
    }
}

}  // namespace

// One direction (slots_ab workgroups, match_ba == nullptr) or both, found as match_q8_pairs finds them.  There is no refusal
// of a one-row side here: a pair's one row is a legitimate candidate set; an empty side leaves -1 / INT32_MIN.
// (waves_per_eu 4: four workgroups per CU as match_q8_pairs has them; left to itself the allocator takes 114 + 16 registers,
// two more than four waves per SIMD leave)
__global__ __launch_bounds__(kPThreads) __attribute__((amdgpu_waves_per_eu(4))) void match_q8_guided_pairs(
    const unsigned char *__restrict__ a, const float *__restrict__ kps_a, const uint64_t *__restrict__ off_a, uint64_t na_total,
    const unsigned char *__restrict__ b, const float *__restrict__ kps_b, const uint64_t *__restrict__ off_b, uint64_t nb_total,
    const float *__restrict__ model, unsigned n_pairs, unsigned slots_ab, unsigned kind, float thr2, float ratio,
    int *__restrict__ match_ab, int *__restrict__ match_ba, int *__restrict__ best_out, int *__restrict__ second_out) {
    __shared__ __attribute__((aligned(16))) Q8GuidedShared sh;
    Q8Slot s;
    if (!q8_pairs_slot(off_a, na_total, off_b, nb_total, n_pairs, slots_ab, s)) return;   // an idle slot
    const bool rev = s.rev;
    const long nx = s.nx, ny = s.ny, block = s.block;
    int *match = (rev ? match_ba : match_ab) + s.out_lo;
    int *best_o = rev || !best_out ? nullptr : best_out + s.out_lo, *second_o = rev || !second_out ? nullptr : second_out + s.out_lo;
    if (ny == 0) {                                               // no row to clamp a request to: no candidate for anybody
        q8_fill_none(match, best_o, second_o, block, nx);
        return;
    }
    const float *m = model + 9 * (size_t)s.p;
    const unsigned char *x = (rev ? b : a) + s.x_lo * 128, *y = (rev ? a : b) + s.y_lo * 128;
    const float *kx = (rev ? kps_b : kps_a) + s.x_lo * 5, *ky = (rev ? kps_a : kps_b) + s.y_lo * 5;
    // (kind and rev are the same for the whole workgroup: a scalar branch; the four bodies share the one LDS block)
    if (kind == 0u) {
        if (!rev) q8_guided_block<0>(x, kx, nx, y, ky, ny, m, thr2, ratio, match, best_o, second_o, block, sh);
        else q8_guided_block<1>(x, kx, nx, y, ky, ny, m, thr2, ratio, match, best_o, second_o, block, sh);
    } else {
        if (!rev) q8_guided_block<2>(x, kx, nx, y, ky, ny, m, thr2, ratio, match, best_o, second_o, block, sh);
        else q8_guided_block<3>(x, kx, nx, y, ky, ny, m, thr2, ratio, match, best_o, second_o, block, sh);
    }
}

void launch_match_q8_guided_pairs(const unsigned char *a, const float *kps_a, const uint64_t *off_a, uint64_t na_total,
                                  const unsigned char *b, const float *kps_b, const uint64_t *off_b, uint64_t nb_total,
                                  const float *model, unsigned n_pairs, unsigned kind, float threshold, float ratio, bool mutual,
                                  int *match_ab, int *match_ba, int *best, int *second, hipStream_t stream) {
    if (n_pairs == 0) return;
    const float thr2 = threshold * threshold;   // as launch_match_guided_pairs and the verifiers form it
    const uint64_t slots_ab = match_q8_pairs_slots(na_total, n_pairs);   // the grid lf_mkd_match_q8_pairs_plan reports
    const uint64_t slots = slots_ab + (match_ba ? match_q8_pairs_slots(nb_total, n_pairs) : 0);
    hipLaunchKernelGGL(match_q8_guided_pairs, dim3((unsigned)slots), dim3(kPThreads), 0, stream, a, kps_a, off_a, na_total, b,
                       kps_b, off_b, nb_total, model, n_pairs, (unsigned)slots_ab, kind, thr2, ratio, match_ab, match_ba, best,
                       second);
    if (mutual) launch_match_mutual(off_a, na_total, off_b, nb_total, n_pairs, match_ab, match_ba, stream);
}

}  // namespace lfmkd
