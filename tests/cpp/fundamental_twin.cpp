// Host twin of the fundamental-matrix verifier of local-features_amd/csrc/mkd_verify.hip: the kernels' own arithmetic
// (csrc/mkd_fundamental_math.h, compiled here by a plain C++ compiler with -ffp-contract=off) under a serial restatement of
// what ransac_score and ransac_select do with FundamentalModel -- every sample's candidates and counts, the selection on (count, -c), and the refit with the
// workgroup's summation order (thread tid adds rows tid, tid + 256, ...; an xor butterfly 32 .. 1 within each wave of 64;
// then waves 0 .. 3 in order).  No arithmetic of its own beyond those sums.  tests/fundamental_twin.py drives it:
//
//   fundamental_twin IN OUT      IN = records, each starting with a u32 kind; OUT = their results back to back
//
//   kind 1, whole calls: u32 na, nb, m, n_seeds, n_hyp, flags, want_records; f32 thr; VerifyPair; f32 ka[na][5], kb[nb][5];
//       i32 match[na], list[m]; u32 seed_p[n_seeds].  For every seed: f32 F[9], u32 stats[4], i32 verified[na], and with
//       want_records for every sample k < n_hyp: u32 pos[7], valid bits, f32 f[3][9], fn[3][9], u32 count[3] (0xFFFFFFFF
//       for an invalid candidate).
//   kind 2, cubic_roots alone: u32 n; f32 c[n][4] (c0 .. c3) -> per cubic u32 roots, f32 x[3].
//   kind 3, null_space alone: u32 n; f32 A[n][7][9] -> per system u32 ok, f32 F1[9], F2[9].
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "mkd_fundamental_math.h"

using namespace lfmkd;

namespace {

constexpr int kThreads = 256, kWave = 64, kWaves = kThreads / kWave;

template <typename T>
void get(FILE *f, T *p, size_t n) {
    if (n && fread(p, sizeof(T), n, f) != n) {
        fprintf(stderr, "fundamental_twin: input ends early\n");
        exit(2);
    }
}
template <typename T>
void put(FILE *f, const T *p, size_t n) {
    if (n && fwrite(p, sizeof(T), n, f) != n) {
        fprintf(stderr, "fundamental_twin: cannot write\n");
        exit(2);
    }
}

// block_sum of mkd_scene.h over per-thread values v[thread][N]
template <typename T>
void block_sum(const T *v, int N, T *total) {
    std::vector<T> cur(kThreads), nxt(kThreads);
    for (int i = 0; i < N; ++i) {
        for (int t = 0; t < kThreads; ++t) cur[t] = v[size_t(t) * N + i];
        for (int o = 32; o > 0; o >>= 1) {
            for (int t = 0; t < kThreads; ++t) nxt[t] = cur[t] + cur[t ^ o];
            cur.swap(nxt);
        }
        T s = cur[0];
        for (int w = 1; w < kWaves; ++w) s += cur[w * kWave];
        total[i] = s;
    }
}

struct Problem {
    unsigned na, nb, n_hyp, flags;
    float thr2;
    VerifyPair P;
    std::vector<float> ka, kb;
    std::vector<int> match, list;

    // load_row of mkd_verify_common.h
    bool row(uint64_t r, float &ax, float &ay, float &bx, float &by) const {
        const int m = match[r];
        if (m < 0 || uint64_t(m) >= nb) return false;
        ax = ka[5 * r];
        ay = ka[5 * r + 1];
        bx = kb[5 * uint64_t(m)];
        by = kb[5 * uint64_t(m) + 1];
        return true;
    }
};

struct Record {
    unsigned pos[7], valid;
    float f[3][9], fn[3][9];
    unsigned count[3];
};

void run(const Problem &q, unsigned seed_p, bool want_records, FILE *out) {
    const float *ka = q.ka.data(), *kb = q.kb.data();
    const int *mt = q.match.data(), *list = q.list.data();
    const unsigned na = q.na;
    const float thr2 = q.thr2;
    // ransac_score, summed over the slices; ransac_select's argmax on (count, -c), an invalid candidate skipped
    std::vector<Record> recs(want_records ? q.n_hyp : 0);
    unsigned long long best = 0;
    for (unsigned k = 0; k < q.n_hyp; ++k) {
        Record rec;
        rec.valid = candidates(ka, kb, mt, list, q.P, seed_p, k, rec.f, rec.fn);
        sample7(seed_p, k, q.P.m, rec.pos);
        unsigned cnt[3] = {0u, 0u, 0u};
        if (rec.valid)
            for (uint64_t r = 0; r < na; ++r) {
                float ax, ay, bx, by;
                if (!q.row(r, ax, ay, bx, by)) continue;
                for (int u = 0; u < 3; ++u) cnt[u] += f_inlier(rec.f[u], ax, ay, bx, by, thr2);
            }
        for (unsigned u = 0; u < 3; ++u) {
            rec.count[u] = (rec.valid >> u) & 1u ? cnt[u] : kInvalid;
            if (rec.count[u] == kInvalid) continue;
            const unsigned c = 3 * k + u;
            const unsigned long long key = ((unsigned long long)(rec.count[u] + 1u) << 32) | (unsigned long long)(kInvalid - c);
            best = key > best ? key : best;
        }
        if (want_records) recs[k] = rec;
    }
    const bool found = best != 0;
    const unsigned c_best = found ? kInvalid - unsigned(best & 0xFFFFFFFFull) : kInvalid;
    const unsigned best_count = found ? unsigned(best >> 32) - 1u : 0u;
    float f[9], fn[9];
    bool have = false;
    {
        float fa[3][9], fna[3][9];
        const unsigned k_best = found ? c_best / 3u : 0u, j_best = found ? c_best % 3u : 0u;
        const unsigned ok = found ? candidates(ka, kb, mt, list, q.P, seed_p, k_best, fa, fna) : 0u;
        have = (ok >> j_best) & 1u;
        for (int i = 0; i < 9; ++i) {
            f[i] = fa[j_best][i];
            fn[i] = fna[j_best][i];
        }
    }
    const VerifyPair &P = q.P;
    unsigned final_count = 0;
    if (have) {
        const bool refine = !(q.flags & 1u);
        std::vector<double> m(size_t(kThreads) * kMoments, 0.0), cost_t(kThreads, 0.0);
        std::vector<unsigned> n_t(kThreads, 0u);
        for (int tid = 0; tid < kThreads; ++tid)
            for (uint64_t r = tid; r < na; r += kThreads) {
                float ax, ay, bx, by, e;
                if (!q.row(r, ax, ay, bx, by)) continue;
                const bool in = f_inlier_cost(f, ax, ay, bx, by, thr2, e);
                cost_t[tid] += e;
                if (!in) continue;
                ++n_t[tid];
                if (refine)
                    add_moments36(&m[size_t(tid) * kMoments], double((ax - P.ca[0]) * P.sa), double((ay - P.ca[1]) * P.sa),
                                  double((bx - P.cb[0]) * P.sb), double((by - P.cb[1]) * P.sb));
            }
        unsigned n_cur;
        double cost_cur;
        block_sum(n_t.data(), 1, &n_cur);
        block_sum(cost_t.data(), 1, &cost_cur);
        for (int round = 0; refine && round < 3; ++round) {
            double ms[kMoments];
            block_sum(m.data(), kMoments, ms);
            float fn2[9], f2[9];
            if (!refit_solve(ms, argmax_abs9(fn), fn2) || !f_denormalise(fn2, P, f2)) break;
            std::fill(m.begin(), m.end(), 0.0);
            std::vector<unsigned> c_t(size_t(kThreads) * 2, 0u);
            std::fill(cost_t.begin(), cost_t.end(), 0.0);
            for (int tid = 0; tid < kThreads; ++tid)
                for (uint64_t r = tid; r < na; r += kThreads) {
                    float ax, ay, bx, by, e;
                    if (!q.row(r, ax, ay, bx, by)) continue;
                    const bool in_old = f_inlier(f, ax, ay, bx, by, thr2);
                    const bool in_new = f_inlier_cost(f2, ax, ay, bx, by, thr2, e);
                    cost_t[tid] += e;
                    c_t[2 * tid + 1] += in_old != in_new;
                    if (!in_new) continue;
                    ++c_t[2 * tid];
                    add_moments36(&m[size_t(tid) * kMoments], double((ax - P.ca[0]) * P.sa), double((ay - P.ca[1]) * P.sa),
                                  double((bx - P.cb[0]) * P.sb), double((by - P.cb[1]) * P.sb));
                }
            unsigned c[2];
            double cost;
            block_sum(c_t.data(), 2, c);
            block_sum(cost_t.data(), 1, &cost);
            if (cost > cost_cur) break;   // a refit whose MSAC cost rises is not kept
            for (int i = 0; i < 9; ++i) {
                f[i] = f2[i];
                fn[i] = fn2[i];
            }
            n_cur = c[0];
            cost_cur = cost;
            if (c[1] == 0) break;         // the inlier set stopped changing
        }
        final_count = n_cur;
    }
    float F[9];
    {
        const int c = argmax_abs9(f);
        for (int i = 0; i < 9; ++i) F[i] = have ? f[i] / f[c] : 0.f;
    }
    const unsigned st[4] = {have ? final_count : 0u, have ? best_count : 0u, have ? c_best : kInvalid, P.m};
    std::vector<int> ver(na);
    for (uint64_t r = 0; r < na; ++r) {
        float ax, ay, bx, by;
        ver[r] = have && q.row(r, ax, ay, bx, by) && f_inlier(f, ax, ay, bx, by, thr2) ? mt[r] : -1;
    }
    put(out, F, 9);
    put(out, st, 4);
    put(out, ver.data(), na);
    for (const Record &rec : recs) {
        put(out, rec.pos, 7);
        put(out, &rec.valid, 1);
        put(out, &rec.f[0][0], 27);
        put(out, &rec.fn[0][0], 27);
        put(out, rec.count, 3);
    }
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: fundamental_twin IN OUT\n");
        return 2;
    }
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) {
        fprintf(stderr, "fundamental_twin: cannot open %s\n", in ? argv[2] : argv[1]);
        return 2;
    }
    static_assert(sizeof(VerifyPair) == 32, "VerifyPair is 6 floats and 2 words");
    unsigned kind;
    while (fread(&kind, sizeof kind, 1, in) == 1) {
        if (kind == 1) {
            unsigned h[7];
            float thr;
            get(in, h, 7);
            get(in, &thr, 1);
            Problem q;
            q.na = h[0], q.nb = h[1], q.n_hyp = h[4], q.flags = h[5];
            q.thr2 = thr * thr;   // as launch_fundamental squares it
            get(in, &q.P, 1);
            q.ka.resize(5 * size_t(q.na));
            q.kb.resize(5 * size_t(q.nb));
            q.match.resize(q.na);
            q.list.resize(h[2]);
            std::vector<unsigned> seeds(h[3]);
            get(in, q.ka.data(), q.ka.size());
            get(in, q.kb.data(), q.kb.size());
            get(in, q.match.data(), q.match.size());
            get(in, q.list.data(), q.list.size());
            get(in, seeds.data(), seeds.size());
            if (q.P.m != h[2]) {
                fprintf(stderr, "fundamental_twin: VerifyPair.m is not the list's length\n");
                return 2;
            }
            for (unsigned s : seeds) run(q, s, h[6] != 0, out);
        } else if (kind == 2) {
            unsigned n;
            get(in, &n, 1);
            for (unsigned i = 0; i < n; ++i) {
                float c[4], x[3];
                get(in, c, 4);
                const unsigned roots = unsigned(cubic_roots(c[0], c[1], c[2], c[3], x));
                put(out, &roots, 1);
                put(out, x, 3);
            }
        } else if (kind == 3) {
            unsigned n;
            get(in, &n, 1);
            for (unsigned i = 0; i < n; ++i) {
                float A[7][9], F1[9], F2[9];
                get(in, &A[0][0], 63);
                const unsigned ok = null_space(A, F1, F2);
                put(out, &ok, 1);
                put(out, F1, 9);
                put(out, F2, 9);
            }
        } else {
            fprintf(stderr, "fundamental_twin: unknown record kind %u\n", kind);
            return 2;
        }
    }
    return fclose(out) == 0 ? 0 : 2;
}
