// Builds the constants of the MKD path on the host (once per handle).
// Formulas follow the reference's LUT builders, local_features/src/mkd_ref.rs:146-267, and its
// upload step, local_features/src/vulkan/mod.rs:1594-1619; the layouts are this library's own.
#include "mkd_consts.hpp"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace lfmkd {

namespace {

// von-Mises Fourier coefficients, mkd_ref.rs:7-9
const float kVmN3K8[4] = {0.37872374f, 0.51796234f, 0.46882015f, 0.39798096f};
const float kVmN1K1[2] = {0.618176f, 0.6934725f};
const float kVmN2K8[3] = {0.37872374f, 0.51796234f, 0.46882015f};

struct Grid {
    float x[kPx], y[kPx];
    Grid() {  // mkd_ref.rs:173-185
        for (int r = 0; r < kPatch; ++r)
            for (int c = 0; c < kPatch; ++c) {
                x[r * kPatch + c] = 2.f * float(c) / float(kPatch - 1) - 1.f;
                y[r * kPatch + c] = 2.f * float(r) / float(kPatch - 1) - 1.f;
            }
    }
};

// component a of the (2n+1)-vector [c0, c_k cos(k t), c_k sin(k t)], mkd_ref.rs:146-171
float vm_component(const float *coef, int n, int a, float t) {
    if (a == 0) return coef[0];
    if (a <= n) return std::cos(t * float(a)) * coef[a];
    return std::sin(t * float(a - n)) * coef[a - n];
}

uint16_t f16_bits(float v) {
    _Float16 h = static_cast<_Float16>(v);  // round to nearest even
    uint16_t b;
    std::memcpy(&b, &h, 2);
    return b;
}
float f16_value(uint16_t b) {
    _Float16 h;
    std::memcpy(&h, &b, 2);
    return static_cast<float>(h);
}

// nearest e2m3 code of |v| <= 7.5 (6 bits: sign, 2 exponent, 3 mantissa; no infinities, no NaNs), ties to the even code
uint32_t e2m3_bits(float v) {
    const float a = std::fabs(v);
    int best = 0;
    float best_d = 1e30f;
    for (int c = 0; c < 32; ++c) {
        const int e = c >> 3, m = c & 7;
        const float val = e == 0 ? float(m) / 8.f : (1.f + float(m) / 8.f) * float(1 << (e - 1));
        const float d = std::fabs(val - a);
        if (d < best_d || (d == best_d && (c & 1) == 0)) {
            best_d = d;
            best = c;
        }
    }
    return uint32_t(best) | (v < 0.f ? 32u : 0u);
}

// One column of the LUT: which spatial kernel, rotated by which harmonic of phi.
struct LutColumn {
    bool used;
    bool polar;     // EP or EC
    int j;          // kernel index within EP / EC
    int k;          // harmonic (von-Mises coefficient c_k; 0 for the m stream)
    int rot;        // 0: as is, 1: times cos(k phi), 2: times sin(k phi)
};

// ---- the unfolded row form (LF_MKD_POOL_F16_FP6 alone): 15 LUT tiles over a row's 32 pixels ----
LutColumn unfolded_lut_column(int ut, int c) {
    LutColumn z{false, false, 0, 0, 0};
    if (ut == 0) return {true, true, c, 0, 0};                                        // m: EP 0..15
    if (ut == 1) return c < 9 ? LutColumn{true, true, 16 + c, 0, 0} : LutColumn{true, false, c - 9, 0, 0};   // EP 16..24 | EC 0..6
    if (ut == 2) return c < 2 ? LutColumn{true, false, 7 + c, 0, 0} : z;               // EC 7, 8
    const int k = (ut - 3) / 4 + 1, part = (ut - 3) % 4;
    if (part == 0) return {true, true, c, k, 1};                                       // P0
    if (part == 1) return {true, true, c, k, 2};                                       // Q0
    if (part == 2) return c < 9 ? LutColumn{true, true, 16 + c, k, 1} : LutColumn{true, false, c - 9, k, 0};   // R
    if (c < 9) return {true, true, 16 + c, k, 2};                                      // S
    return c < 11 ? LutColumn{true, false, 7 + (c - 9), k, 0} : z;
}

// Packed output column (tile after the epilogue's combine step, slot) -> descriptor index, or -1.
// Descriptor order (shaders/common.glsl:114-139): polar block [in-dim i][kernel j] (175), then cartesian [i][j] (63);
// in-dims: 0 = m, k = cos k, k + 3 = sin k.
int unfolded_packed_desc(int tile, int c) {
    const int cart0 = kDimsIn * kPolar;
    if (tile == 0) return c;
    if (tile == 1) return c < 9 ? 16 + c : cart0 + (c - 9);
    if (tile == 2) return c < 2 ? cart0 + 7 + c : -1;
    const int k = (tile - 3) / 6 + 1, part = (tile - 3) % 6;
    const int ic = k, is = k + 3;
    switch (part) {
        case 0: return ic * kPolar + c;
        case 1: return is * kPolar + c;
        case 2: return c < 9 ? ic * kPolar + 16 + c : cart0 + ic * kCart + (c - 9);
        case 3: return c < 9 ? is * kPolar + 16 + c : cart0 + is * kCart + (c - 9);
        case 4: return (c == 9 || c == 10) ? cart0 + ic * kCart + 7 + (c - 9) : -1;
        default: return (c == 9 || c == 10) ? cart0 + is * kCart + 7 + (c - 9) : -1;
    }
}

// ---- the folded row form (LF_MKD_POOL_F16X3, LF_MKD_POOL_F32; mkd_consts.hpp) ----
// One column of a folded LUT tile: what its two K halves hold and which descriptor entries its products are.
struct FoldColumn {
    LutColumn first{false, false, 0, 0, 0}, second{false, false, 0, 0, 0};   // (.used == false: zeros)
    int sign_second = 1;              // the second half is stored times this
    int desc_u = -1, desc_v = -1;     // entry under the operand M or U / under V
    int sign_v = 1;                   // the V product is sign_v x its entry
};
struct FoldLayout {
    FoldColumn col[kUniqueTiles][kTileCols];
};

// parity(col) = +1 / -1: the column is even / odd under x -> 31 - x.  Returns "" or why the layout does not fit.
template <class Parity>
std::string build_fold_layout(Parity parity, FoldLayout &fl) {
    const int cart0 = kDimsIn * kPolar;
    auto place_cart = [&](int ut0, int k, int dc, int ds) -> std::string {   // even EC -> tile 1 slots 10.., odd EC -> tile 2
        int n_even = 0, n_odd = 0;
        for (int i = 0; i < kCart; ++i) {
            const LutColumn ec{true, false, i, k, 0};
            FoldColumn fc;
            if (parity(ec) > 0) {
                if (kPolarSlots + n_even >= kTileCols) return "internal: too many even cartesian kernels for a mixed tile";
                fc.first = ec;
                fc.desc_u = cart0 + dc * kCart + i;
                if (k) fc.desc_v = cart0 + ds * kCart + i;
                fl.col[ut0 + 1][kPolarSlots + n_even++] = fc;
            } else {
                if (n_odd >= kTileCols) return "internal: too many odd cartesian kernels for a tile";
                fc.second = ec;
                fc.desc_u = cart0 + (k ? ds : dc) * kCart + i;   // U's second half is sin_o, M's is m_o
                if (k) { fc.desc_v = cart0 + dc * kCart + i; fc.sign_v = -1; }   // V's is -cos_o
                fl.col[ut0 + 2][n_odd++] = fc;
            }
        }
        return "";
    };
    // m stream: EP 0-15 | EP 16-24 and even EC | odd EC
    for (int j = 0; j < kPolar; ++j) {
        const LutColumn ep{true, true, j, 0, 0};
        FoldColumn fc;
        (parity(ep) > 0 ? fc.first : fc.second) = ep;
        fc.desc_u = j;
        if (j >= kTileCols + kPolarSlots) return "internal: the m stream's polar kernels do not fit two tiles";
        fl.col[j / kTileCols][j % kTileCols] = fc;
    }
    if (const std::string e = place_cart(0, 0, 0, 0); !e.empty()) return e;
    for (int k = 1; k <= 3; ++k) {
        const int ut0 = 3 + 3 * (k - 1), ic = k, is = k + 3;
        FoldColumn cls[2][kPolar];   // [0]: EPc even, [1]: EPc odd
        int n[2] = {0, 0};
        for (int j = 0; j < kPolar; ++j) {
            const LutColumn pc{true, true, j, k, 1}, ps{true, true, j, k, 2};
            if (parity(pc) == parity(ps)) return "internal: EP cos and EP sin columns of equal parity";
            FoldColumn fc;
            if (parity(pc) > 0) {
                fc.first = pc; fc.second = ps; fc.sign_second = -1;
                fc.desc_u = ic * kPolar + j; fc.desc_v = is * kPolar + j;
            } else {
                fc.first = ps; fc.second = pc;
                fc.desc_u = is * kPolar + j; fc.desc_v = ic * kPolar + j; fc.sign_v = -1;
            }
            cls[parity(pc) > 0 ? 0 : 1][n[parity(pc) > 0 ? 0 : 1]++] = fc;
        }
        const int big = n[0] >= n[1] ? 0 : 1;
        if (n[big] > kTileCols || n[big ^ 1] > kPolarSlots) return "internal: the polar parity classes do not fit their tiles";
        for (int i = 0; i < n[big]; ++i) fl.col[ut0][i] = cls[big][i];
        for (int i = 0; i < n[big ^ 1]; ++i) fl.col[ut0 + 1][i] = cls[big ^ 1][i];
        if (const std::string e = place_cart(ut0, k, ic, is); !e.empty()) return e;
    }
    return "";
}

// accumulator tile -> (LUT tile, 0: operand M / U, 1: operand V)
void acc_tile_source(int t, int &ut, int &v) {
    if (t < 3) { ut = t; v = 0; return; }
    const int h = (t - 3) / 6, r = (t - 3) % 6;
    ut = 3 + 3 * h + r / 2;
    v = r & 1;
}

}  // namespace

std::string load_pca_safetensors(const std::string &path, PcaModel &out) {
    FILE *f = std::fopen(path.c_str(), "rb");
    if (!f) return "cannot open " + path;
    std::string err;
    uint64_t hlen = 0;
    std::vector<char> hdr;
    if (std::fread(&hlen, 8, 1, f) != 1 || hlen == 0 || hlen > (1u << 20)) err = "bad header length";
    if (err.empty()) {
        hdr.assign(hlen + 1, 0);
        if (std::fread(hdr.data(), 1, hlen, f) != hlen) err = "truncated header";
    }
    auto tensor = [&](const char *name, size_t count, std::vector<float> &dst) {
        if (!err.empty()) return;
        const std::string key = std::string("\"") + name + "\"";
        const char *p = std::strstr(hdr.data(), key.c_str());
        if (p) p = std::strstr(p, "\"data_offsets\"");
        if (p) p = std::strchr(p, '[');
        long b = 0, e = 0;
        if (!p || std::sscanf(p, "[%ld,%ld]", &b, &e) != 2 || size_t(e - b) != count * 4) {
            err = std::string("tensor '") + name + "' missing or of unexpected size";
            return;
        }
        dst.resize(count);
        std::fseek(f, long(8 + hlen) + b, SEEK_SET);
        if (std::fread(dst.data(), 4, count, f) != count) err = "truncated tensor data";
    };
    tensor("mean", kRaw, out.mean);
    tensor("eigvals", kRaw, out.eigvals);
    tensor("eigvecs", size_t(kRaw) * kRaw, out.eigvecs);
    std::fclose(f);
    return err.empty() ? "" : path + ": " + err;
}

std::string build_host_consts(const PcaModel &pca, HostConsts &hc) {
    // The whitening scale is eigvals^-0.35 (mod.rs:1604-1612): a non-positive or non-finite eigenvalue among the 128 it uses,
    // or a non-finite mean / eigenvector entry, would put NaNs into every descriptor.  The reference unwraps its embedded
    // models (mkd_ref.rs:352-391); a caller-supplied model is checked and refused instead.
    if (pca.mean.size() != size_t(kRaw) || pca.eigvals.size() != size_t(kRaw) || pca.eigvecs.size() != size_t(kRaw) * kRaw)
        return "PCA model: mean[238], eigvals[238] and eigvecs[238*238] are required";
    for (int r = 0; r < kOut; ++r)
        if (!(pca.eigvals[r] > 0.f) || !std::isfinite(pca.eigvals[r]))
            return "PCA model: eigvals[" + std::to_string(r) + "] must be positive and finite (the whitening scales by eigvals^-0.35)";
    for (float v : pca.mean)
        if (!std::isfinite(v)) return "PCA model: mean holds a non-finite value";
    for (float v : pca.eigvecs)
        if (!std::isfinite(v)) return "PCA model: eigvecs holds a non-finite value";
    static const Grid grid;
    const float kPi = 3.14159265358979323846f, kSqrt2 = 1.41421356237309504880f;

    // gradient_angle = -atan2(y, x) of the pixel grid; rho with its epsilon (mkd_ref.rs:133-144)
    hc.gradient_angle.resize(kPx);
    std::vector<float> rho(kPx), gauss(kPx);
    float max_norm = 0.f;
    for (int p = 0; p < kPx; ++p) {
        hc.gradient_angle[p] = -std::atan2(grid.y[p], grid.x[p]);
        rho[p] = std::sqrt(grid.x[p] * grid.x[p] + grid.y[p] * grid.y[p] + 1e-8f);
        max_norm = std::fmax(max_norm, std::sqrt(grid.x[p] * grid.x[p] + grid.y[p] * grid.y[p]));
    }
    for (int p = 0; p < kPx; ++p) {  // mkd_ref.rs:259-267, sigma = 1
        const float nn = std::sqrt(grid.x[p] * grid.x[p] + grid.y[p] * grid.y[p]) / max_norm;
        gauss[p] = std::exp((nn * nn) / -1.f);
    }
    // EC[a*3+b] = vM1(x pi/2)[a] vM1(y pi/2)[b] G   (mkd_ref.rs:210-231, mod.rs:1614-1615)
    hc.embedding_cartesian.resize(size_t(kCart) * kPx);
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b)
            for (int p = 0; p < kPx; ++p) {
                const float ea = vm_component(kVmN1K1, 1, a, grid.x[p] * (kPi / 2.f));
                const float eb = vm_component(kVmN1K1, 1, b, grid.y[p] * (kPi / 2.f));
                hc.embedding_cartesian[size_t(a * 3 + b) * kPx + p] = (ea * eb) * gauss[p];
            }
    // EP[a*5+b] = vM2(+atan2)[a] vM2(rho pi/sqrt2)[b] G   (mkd_ref.rs:233-257, mod.rs:1616-1617)
    hc.embedding_polar.resize(size_t(kPolar) * kPx);
    for (int a = 0; a < 5; ++a)
        for (int b = 0; b < 5; ++b)
            for (int p = 0; p < kPx; ++p) {
                const float ea = vm_component(kVmN2K8, 2, a, hc.gradient_angle[p] * -1.f);
                const float eb = vm_component(kVmN2K8, 2, b, rho[p] * kPi / kSqrt2);
                hc.embedding_polar[size_t(a * 5 + b) * kPx + p] = (ea * eb) * gauss[p];
            }
    // W_T[r][c] = eigvecs[c][r] * eigvals[r]^(-0.35)   (mod.rs:1604-1612)
    hc.mean = pca.mean;
    hc.w_t.resize(size_t(kOut) * kRaw);
    const float expo = -0.5f * 0.7f;
    for (int r = 0; r < kOut; ++r) {
        const float s = std::pow(pca.eigvals[r], expo);
        for (int c = 0; c < kRaw; ++c) hc.w_t[size_t(r) * kRaw + c] = pca.eigvecs[size_t(c) * kRaw + r] * s;
    }

    // ---- device layouts ----
    auto lut_value_d = [&](const LutColumn &col, int px) -> double {
        if (!col.used) return 0.0;
        const double e = col.polar ? hc.embedding_polar[size_t(col.j) * kPx + px]
                                   : hc.embedding_cartesian[size_t(col.j) * kPx + px];
        const double ph = double(col.k) * double(hc.gradient_angle[px]);
        const double rot = col.rot == 1 ? std::cos(ph) : (col.rot == 2 ? std::sin(ph) : 1.0);
        return double(kVmN3K8[col.k]) * e * rot;
    };
    auto lut_value = [&](const LutColumn &col, int px) -> float { return float(lut_value_d(col, px)); };
    // the x-parity of a column, and how far the column is from having one
    float defect = 0.f;
    int known[2][kPolar][4][3] = {};
    auto parity = [&](const LutColumn &col) -> int {
        int &memo = known[col.polar ? 1 : 0][col.j][col.k][col.rot];
        if (memo) return memo;
        double even_err = 0.0, odd_err = 0.0, mx = 0.0;
        for (int y = 0; y < kPatch; ++y)
            for (int x = 0; x < kPatch / 2; ++x) {
                const double a = lut_value(col, y * kPatch + x), b = lut_value(col, y * kPatch + kPatch - 1 - x);
                even_err = std::fmax(even_err, std::fabs(a - b));
                odd_err = std::fmax(odd_err, std::fabs(a + b));
                mx = std::fmax(mx, std::fmax(std::fabs(a), std::fabs(b)));
            }
        defect = std::fmax(defect, float(std::fmin(even_err, odd_err) / mx));
        return memo = even_err <= odd_err ? 1 : -1;
    };
    FoldLayout fl;
    if (const std::string e = build_fold_layout(parity, fl); !e.empty()) return e;
    hc.lut_parity_defect = defect;
    if (!(defect < 1e-4f))   // (f32 rounding of the grid and of atan2 leaves a few 1e-6)
        return "internal: a pooling LUT column is neither even nor odd in x (defect " + std::to_string(defect) + ")";
    // The x-odd Cartesian kernels as c_k fx(x) gy_b(y) (mkd_consts.hpp): LF_MKD_POOL_F16X3 pools them on the vector ALU.
    // f32 rounding of the builder's three factors and of `gauss` leaves a few ulp between the product and the LUT.
    {
        for (int k = 0; k <= 3; ++k)
            for (int i = 0; i < kCart; ++i)
                if ((parity(LutColumn{true, false, i, k, 0}) < 0) != (i >= 6))
                    return "internal: the x-odd cartesian kernels are not EC 6, 7, 8";
        const double half_pi = 3.14159265358979323846 / 2.0, mn2 = double(max_norm) * double(max_norm);
        auto vm1 = [&](int a, double t) {
            return a == 0 ? double(kVmN1K1[0]) : (a == 1 ? std::cos(t) : std::sin(t)) * double(kVmN1K1[1]);
        };
        auto fx = [&](int x) {
            const double g = grid.x[x];
            return vm1(2, g * half_pi) * std::exp(-(g * g) / mn2);
        };
        for (int x = 0; x < kPatch / 2; ++x) hc.odd_cart_fx[x] = float(0.5 * (fx(x) - fx(kPatch - 1 - x)));
        for (int y = 0; y < kPatch; ++y) {
            const double g = grid.y[y * kPatch];
            for (int b = 0; b < 3; ++b) hc.odd_cart_gy[y][b] = float(vm1(b, g * half_pi) * std::exp(-(g * g) / mn2));
            hc.odd_cart_gy[y][3] = 0.f;
        }
        double worst = 0.0;
        for (int k = 0; k <= 3; ++k)
            for (int b = 0; b < 3; ++b) {
                const LutColumn col{true, false, 6 + b, k, 0};
                double err = 0.0, mx = 0.0;
                for (int y = 0; y < kPatch; ++y)
                    for (int x = 0; x < kPatch; ++x) {
                        const double f = x < kPatch / 2 ? hc.odd_cart_fx[x] : -double(hc.odd_cart_fx[kPatch - 1 - x]);
                        const double v = lut_value_d(col, y * kPatch + x);
                        err = std::fmax(err, std::fabs(double(kVmN3K8[k]) * f * double(hc.odd_cart_gy[y][b]) - v));
                        mx = std::fmax(mx, std::fabs(v));
                    }
                worst = std::fmax(worst, err / mx);
            }
        hc.odd_cart_defect = float(worst);
        if (!(hc.odd_cart_defect < 1e-6f))
            return "internal: the x-odd cartesian kernels are not a product of an x- and a y-profile (defect " +
                   std::to_string(hc.odd_cart_defect) + ")";
    }
    hc.colmap.assign(kPackedCols, -1);
    {
        std::vector<int> seen(kRaw, 0);
        for (int t = 0; t < kTiles; ++t) {
            int ut, v;
            acc_tile_source(t, ut, v);
            for (int c = 0; c < kTileCols; ++c) {
                const FoldColumn &fc = fl.col[ut][c];
                const int d = v ? fc.desc_v : fc.desc_u;
                if (d < 0) continue;
                hc.colmap[t * kTileCols + c] = int16_t(v && fc.sign_v < 0 ? -2 - d : d);
                ++seen[d];
            }
        }
        for (int d = 0; d < kRaw; ++d)
            if (seen[d] != 1)   // every descriptor entry has exactly one packed column
                return "internal: descriptor entry " + std::to_string(d) + " has " + std::to_string(seen[d]) + " packed columns";
    }
    hc.pool_b_f32.assign(size_t(kPatch) * kUniqueTiles * 2 * 64 * 4, 0.f);
    hc.pool_b_f16.assign(size_t(kPatch) * kUniqueTiles * 2 * 64 * 8, 0);
    for (int y = 0; y < kPatch; ++y)
        for (int ut = 0; ut < kUniqueTiles; ++ut)
            for (int lane = 0; lane < 64; ++lane) {
                const FoldColumn &fc = fl.col[ut][lane & 15];
                const int q = lane >> 4;
                for (int e = 0; e < 8; ++e) {
                    const LutColumn &col = e < 4 ? fc.first : fc.second;
                    float v = 0.f;
                    if (col.used) {   // the mean of the two mirror values, in f64
                        const int x = 4 * q + (e & 3);
                        const double a = lut_value_d(col, y * kPatch + x), b = lut_value_d(col, y * kPatch + kPatch - 1 - x);
                        v = float(0.5 * (a + double(parity(col)) * b) * double(e < 4 ? 1 : fc.sign_second));
                    }
                    hc.pool_b_f32[(((size_t(y) * kUniqueTiles + ut) * 2 + (e >> 2)) * 64 + lane) * 4 + (e & 3)] = v;
                    const uint16_t hi = f16_bits(v);
                    const uint16_t lo = f16_bits(v - f16_value(hi));  // f16 subnormals survive the MFMA (tools/micro)
                    hc.pool_b_f16[(((size_t(y) * kUniqueTiles + ut) * 2 + 0) * 64 + lane) * 8 + e] = hi;
                    hc.pool_b_f16[(((size_t(y) * kUniqueTiles + ut) * 2 + 1) * 64 + lane) * 8 + e] = lo;
                }
            }
    // LF_MKD_POOL_F16_FP6: the unfolded row images, with the cross-term operands of the harmonics' tiles (see mkd_consts.hpp)
    hc.colmap_unfolded.assign(kPackedCols, -1);
    for (int t = 0; t < kTiles; ++t)
        for (int c = 0; c < kTileCols; ++c) hc.colmap_unfolded[t * kTileCols + c] = int16_t(unfolded_packed_desc(t, c));
    hc.pool_b_fp6.assign(size_t(kPatch) * kUnfUniqueTiles * 2 * 64 * 8, 0);
    for (int y = 0; y < kPatch; ++y)
        for (int ut = 0; ut < kUnfUniqueTiles; ++ut)
            for (int lane = 0; lane < 64; ++lane) {
                const LutColumn col = unfolded_lut_column(ut, lane & 15);
                const int q = lane >> 4;
                for (int e = 0; e < 8; ++e) {
                    const float v = lut_value(col, y * kPatch + 8 * q + e);
                    const uint16_t hi = f16_bits(v);
                    hc.pool_b_fp6[(((size_t(y) * kUnfUniqueTiles + ut) * 2 + 0) * 64 + lane) * 8 + e] = hi;
                    hc.pool_b_fp6[(((size_t(y) * kUnfUniqueTiles + ut) * 2 + 1) * 64 + lane) * 8 + e] = f16_bits(v - f16_value(hi));
                }
            }
    {
        const float kX = 2048.f;      // the residuals' common factor (the kernel scales its stream residuals by the same)
        auto slot_values = [&](int y, int ut, int lane, float (&sv)[16]) {
            const LutColumn col = unfolded_lut_column(ut, lane & 15);
            const int q = lane >> 4;
            for (int e = 0; e < 8; ++e) {
                const float v = lut_value(col, y * kPatch + 8 * q + e);
                const float hi = f16_value(f16_bits(v));
                sv[2 * e] = kX * (v - hi);
                sv[2 * e + 1] = hi;
            }
        };
        for (int y = 0; y < kPatch; ++y)
            for (int ut = 3; ut < kUnfUniqueTiles; ++ut)
                for (int lane = 0; lane < 64; ++lane) {
                    float sv[16], other[16];
                    slot_values(y, ut, lane, sv);
                    float mx = 0.f;
                    for (float v : sv) mx = std::fmax(mx, std::fabs(v));
                    const int part = (ut - 3) % 4;
                    if (part < 2) {   // P0 and Q0 of a harmonic share the scale
                        slot_values(y, part == 0 ? ut + 1 : ut - 1, lane, other);
                        for (float v : other) mx = std::fmax(mx, std::fabs(v));
                    }
                    int ex = 0;                                   // T = 2^ex with mx / T in [2, 4)
                    if (mx > 0.f) ex = int(std::floor(std::log2(mx))) - 1;
                    const float inv_t = std::ldexp(1.f, -ex);
                    uint32_t w[4] = {0u, 0u, 0u, uint32_t(127 + ex) & 255u};
                    for (int f = 0; f < 16; ++f) {
                        const uint64_t bits = uint64_t(e2m3_bits(sv[f] * inv_t)) << ((6 * f) & 31);
                        w[(6 * f) / 32] |= uint32_t(bits);
                        if ((6 * f) / 32 + 1 < 3) w[(6 * f) / 32 + 1] |= uint32_t(bits >> 32);
                    }
                    uint16_t *dst = &hc.pool_b_fp6[(((size_t(y) * kUnfUniqueTiles + ut) * 2 + 1) * 64 + lane) * 8];
                    std::memcpy(dst, w, 16);
                }
    }
    // whitening fragments in a packed order (colmap: the folded forms; colmap_unfolded: LF_MKD_POOL_F16_FP6)
    auto w_packed = [&](const std::vector<int16_t> &cm, int n, int packed_col) -> float {
        const int d = packed_col < kPackedCols ? cm[packed_col] : -1;
        if (d == -1) return 0.f;
        return d >= 0 ? hc.w_t[size_t(n) * kRaw + d] : -hc.w_t[size_t(n) * kRaw + (-2 - d)];
    };
    auto white_f16 = [&](const std::vector<int16_t> &cm, std::vector<uint16_t> &dst) {
        dst.assign(size_t(11) * 8 * 2 * 64 * 8, 0);
        for (int r = 0; r < 8; ++r)
            for (int lane = 0; lane < 64; ++lane) {
                const int n = 16 * r + (lane & 15), q = lane >> 4;
                for (int s = 0; s < 11; ++s)
                    for (int j = 0; j < 8; ++j) {
                        const float v = w_packed(cm, n, 16 * (2 * s + (j >> 2)) + 4 * q + (j & 3));
                        const uint16_t hi = f16_bits(v);
                        dst[(((size_t(s) * 8 + r) * 2 + 0) * 64 + lane) * 8 + j] = hi;
                        dst[(((size_t(s) * 8 + r) * 2 + 1) * 64 + lane) * 8 + j] = f16_bits(v - f16_value(hi));
                    }
            }
    };
    white_f16(hc.colmap, hc.white_a_f16);
    white_f16(hc.colmap_unfolded, hc.white_a_f16_unfolded);
    hc.white_a_f32.assign(size_t(kTiles) * 4 * 8 * 64, 0.f);
    for (int r = 0; r < 8; ++r)
        for (int lane = 0; lane < 64; ++lane) {
            const int n = 16 * r + (lane & 15), q = lane >> 4;
            for (int t = 0; t < kTiles; ++t)
                for (int i = 0; i < 4; ++i)
                    hc.white_a_f32[((size_t(t) * 4 + i) * 8 + r) * 64 + lane] = w_packed(hc.colmap, n, 16 * t + 4 * q + i);
        }
    hc.white_bias.assign(kOut, 0.f);
    for (int n = 0; n < kOut; ++n) {
        double b = 0.0;
        for (int d = 0; d < kRaw; ++d) b -= double(hc.w_t[size_t(n) * kRaw + d]) * double(pca.mean[d]);
        hc.white_bias[n] = float(b);
    }
    return "";
}

}  // namespace lfmkd
