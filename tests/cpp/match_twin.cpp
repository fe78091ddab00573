// Host twin of the screen matcher's decision (match_verify in local-features_amd/csrc/mkd_match.hip): an exhaustive scan
// of every (a row, b row) pair with verify's own f32 dot product, best / second / index under verify's rule.  The screen
// form promises exactly this for every row it does not hand to the fallback scan (include/lf_mkd.h), so the device is held
// to this program bit for bit by tests/test_gpu_match_exact.py.
//
// The dot product, as the kernel takes it: 16 lanes, lane l owns elements 8 l .. 8 l + 7 of the two rows,
//   p_l = a[8l] * b[8l];  p_l = fmaf(a[8l + j], b[8l + j], p_l)  for j = 1 .. 7
// then p_l += p_{l ^ 8}, ^ 4, ^ 2, ^ 1, all in f32.  f32 addition is commutative, so every lane ends with lane 0's value
// and the tree is restated on the lower half alone.  fmaf is the C library's (correctly rounded, a hardware fma where the
// processor has one); nothing here may be contracted or reassociated: build with -O2 -ffp-contract=off, never -ffast-math.
//
// usage: match_twin <problem file> <result file>; all little endian
//   problem: u32 magic 'MTW1', u32 na, u32 nb, u32 flags (1: exclusion ranges follow, 2: float64 results wanted),
//            f32 ratio, u32 threads (at most 16 are used); a [na][128] f32; b [nb][128] f32; lo [na] u32, hi [na] u32 if flag 1
//   result:  match [na] i32, best [na] f32, second [na] f32; with flag 2 also best [na] f64, second [na] f64 (the two largest
//            float64 similarities of the row, chosen in float64) and sabs [na] f64 (the row's largest sum |a_k b_k|)
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <thread>
#include <vector>

namespace {

constexpr uint32_t kMagic = 0x3157544du;   // "MTW1"
constexpr int kDim = 128;

struct Problem {
    uint32_t na = 0, nb = 0, flags = 0, threads = 1;
    float ratio = 0.f;
    std::vector<float> a, b;
    std::vector<uint32_t> lo, hi;
};

struct Result {
    std::vector<int32_t> match;
    std::vector<float> best, second;
    std::vector<double> best64, second64, sabs;
};

// match_verify's dot product of two rows
inline __attribute__((always_inline)) float dot(const float *a, const float *b) {
    float p[16];
    for (int l = 0; l < 16; ++l) {
        float q = a[8 * l] * b[8 * l];
        for (int j = 1; j < 8; ++j) q = std::fmaf(a[8 * l + j], b[8 * l + j], q);
        p[l] = q;
    }
    for (int m = 8; m >= 1; m >>= 1)
        for (int l = 0; l < m; ++l) p[l] = p[l] + p[l ^ m];
    return p[0];
}

// the same pairs in float64: the products are exact, the sum is pairwise (8 per lane, then the tree); s = sum |a_k b_k|
inline __attribute__((always_inline)) double dot64(const float *a, const float *b, double &s) {
    double p[16], t[16];
    for (int l = 0; l < 16; ++l) {
        double q = 0.0, u = 0.0;
        for (int j = 0; j < 8; ++j) {
            const double x = (double)a[8 * l + j] * (double)b[8 * l + j];
            q += x;
            u += std::fabs(x);
        }
        p[l] = q;
        t[l] = u;
    }
    for (int m = 8; m >= 1; m >>= 1)
        for (int l = 0; l < m; ++l) { p[l] += p[l ^ m]; t[l] += t[l ^ m]; }
    s = t[0];
    return p[0];
}

// a rows [r0, r1): every b row outside [lo, hi), ascending
__attribute__((target_clones("arch=haswell", "default")))
void scan_rows(const Problem &pr, Result &out, uint32_t r0, uint32_t r1) {
    const bool excl = pr.flags & 1u, wide = pr.flags & 2u;
    const float inf = std::numeric_limits<float>::infinity();
    for (uint32_t i = r0; i < r1; ++i) {
        const float *a = &pr.a[(size_t)i * kDim];
        const uint32_t lo = excl ? pr.lo[i] : 0u, hi = excl ? pr.hi[i] : 0u;
        float e1 = -inf, e2 = -inf;
        int ei = -1;
        double d1 = -(double)inf, d2 = -(double)inf, smax = 0.0;
        for (uint32_t r = 0; r < pr.nb; ++r) {
            if (r >= lo && r < hi) continue;
            const float *b = &pr.b[(size_t)r * kDim];
            const float p = dot(a, b);
            const int row = (int)r;
            const bool nb_ = p > e1 || (p == e1 && row > ei);
            e2 = nb_ ? e1 : std::fmax(e2, p);
            ei = nb_ ? row : ei;
            e1 = nb_ ? p : e1;
            if (wide) {
                double s;
                const double d = dot64(a, b, s);
                if (d > d1) { d2 = d1; d1 = d; }
                else if (d > d2) d2 = d;
                smax = std::max(smax, s);
            }
        }
        const float scaled = e1 * pr.ratio;
        out.match[i] = (ei >= 0 && (pr.ratio <= 0.f || scaled > e2)) ? ei : -1;
        out.best[i] = e1;
        out.second[i] = e2;
        if (wide) { out.best64[i] = d1; out.second64[i] = d2; out.sabs[i] = smax; }
    }
}

template <typename T>
bool read_vec(FILE *f, std::vector<T> &v, size_t n) {
    v.resize(n);
    return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

template <typename T>
bool write_vec(FILE *f, const std::vector<T> &v) {
    return v.empty() || fwrite(v.data(), sizeof(T), v.size(), f) == v.size();
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 3) { fprintf(stderr, "usage: match_twin <problem> <result>\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "match_twin: cannot read %s\n", argv[1]); return 1; }
    Problem pr;
    uint32_t head[4];
    bool ok = fread(head, 4, 4, f) == 4 && head[0] == kMagic && fread(&pr.ratio, 4, 1, f) == 1 &&
              fread(&pr.threads, 4, 1, f) == 1;
    if (ok) {
        pr.na = head[1]; pr.nb = head[2]; pr.flags = head[3];
        ok = read_vec(f, pr.a, (size_t)pr.na * kDim) && read_vec(f, pr.b, (size_t)pr.nb * kDim);
        if (ok && (pr.flags & 1u)) ok = read_vec(f, pr.lo, pr.na) && read_vec(f, pr.hi, pr.na);
    }
    fclose(f);
    if (!ok) { fprintf(stderr, "match_twin: %s is not a problem file\n", argv[1]); return 1; }

    Result out;
    out.match.resize(pr.na); out.best.resize(pr.na); out.second.resize(pr.na);
    if (pr.flags & 2u) { out.best64.resize(pr.na); out.second64.resize(pr.na); out.sabs.resize(pr.na); }
    const uint32_t hw = std::max(1u, std::thread::hardware_concurrency());
    const uint32_t nt = std::max(1u, std::min({pr.threads, 16u, hw, std::max(1u, pr.na / 8)}));
    std::vector<std::thread> pool;
    for (uint32_t t = 1; t < nt; ++t)
        pool.emplace_back(scan_rows, std::cref(pr), std::ref(out), (uint32_t)((uint64_t)pr.na * t / nt),
                          (uint32_t)((uint64_t)pr.na * (t + 1) / nt));
    scan_rows(pr, out, 0, (uint32_t)((uint64_t)pr.na / nt));
    for (auto &t : pool) t.join();

    f = fopen(argv[2], "wb");
    if (!f) { fprintf(stderr, "match_twin: cannot write %s\n", argv[2]); return 1; }
    ok = write_vec(f, out.match) && write_vec(f, out.best) && write_vec(f, out.second) && write_vec(f, out.best64) &&
         write_vec(f, out.second64) && write_vec(f, out.sabs);
    ok = (fclose(f) == 0) && ok;
    if (!ok) { fprintf(stderr, "match_twin: short write to %s\n", argv[2]); return 1; }
    return 0;
}
