// Host-side constants of the MKD path and their device layouts.
//
// What the reference uploads once in upload_constant_data (vulkan/mod.rs:1587-1713) as
// ConstantData (shaders/common.glsl:34-40) is rebuilt here and re-laid-out for the MFMA
// kernels: the spatial kernels become B-operand fragments, the PCA matrix too.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

namespace lfmkd {

constexpr int kPatch = 32;
constexpr int kPx = kPatch * kPatch;
constexpr int kDimsIn = 7;      // shaders/common.glsl:22
constexpr int kCart = 9;        // shaders/common.glsl:23
constexpr int kPolar = 25;      // shaders/common.glsl:24
constexpr int kRaw = 238;       // shaders/common.glsl:33
constexpr int kOut = 128;       // shaders/common.glsl:20

// Pooling as a GEMM: rows = patches, K = pixels, columns = (stream, kernel) pairs.
// A "stream" is one per-pixel operand value; there are SEVEN:
//   0: m | 1..3: m cos(k t) | 4..6: m sin(k t)          (t = gradient angle, m = sqrt(|grad|); embedding.glsl:34-51)
// The reference also embeds the RELATIVE angle t + phi(px) (embedding.glsl:70-77, polar kernels).  phi depends on the
// pixel only, so its rotation is folded into the LUT instead of into six more streams:
//   sum_px m cos(k(t+phi)) EP_j = sum_px [m cos kt] (EP_j cos k phi) - [m sin kt] (EP_j sin k phi)
//   sum_px m sin(k(t+phi)) EP_j = sum_px [m sin kt] (EP_j cos k phi) + [m cos kt] (EP_j sin k phi)
// A patch row is then FOLDED about its middle (the pixel grid's x -> -x): every LUT column L is even or odd in x (to f32
// rounding; build_host_consts checks it), so with e(x) = s(x) + s(31-x), o(x) = s(x) - s(31-x) for x < 16
//   sum_{x<32} L(x) s(x) = sum_{x<16} L(x) e(x)  (L even)   or   sum_{x<16} L(x) o(x)  (L odd),
// and EPc_j = c_k EP_j cos k phi, EPs_j = c_k EP_j sin k phi (c_k the von-Mises coefficient) always have OPPOSITE parity.
// One K = 32 operand therefore holds the even half of one stream beside the odd half of the other:
//   M = [m_e | m_o]      U_k = [cos_e | sin_o]      V_k = [sin_e | -cos_o]
// (K slot of a lane (patch, q): 0-3 = the first half at x = 4q + i, 4-7 = the second half at the same x) and per harmonic
// both operands meet the SAME three LUT tiles, whose columns are one of
//   EPc_j even: [EPc_j | -EPs_j]   U -> relcos_j,  V -> relsin_j
//   EPc_j odd:  [EPs_j |  EPc_j]   U -> relsin_j,  V -> -relcos_j
//   EC_i even:  [EC_i | 0]         U -> abscos_i,  V -> abssin_i
//   EC_i odd:   [0 | EC_i]         U -> abssin_i,  V -> -abscos_i
// The minus signs of the V products are carried by the whitening fragments (and by `colmap` for the raw tap).
// Tiles of a harmonic: 0 = the larger polar class (15 columns) | 1 = the smaller (10, slots 0-9), even EC (6, slots 10-15) |
// 2 = odd EC (3).  The m stream's three tiles have the same shape: EP 0-15 | EP 16-24, even EC in slots 10-15 | odd EC; a
// column fills the half its parity selects.  The LUT is symmetrised: a folded value is the f64 mean of the two mirror values.
// 12 LUT tiles and 21 accumulator tiles per row, 6 products per harmonic; the accumulators are the packed output columns.
// LF_MKD_POOL_F16X3 does not spend matrix instructions on tile 2 of a group ([0 | EC_i], 3 of 16 columns, half of every K
// zero): the x-odd Cartesian kernels are EC 6, 7, 8 = vM1(x pi/2)[2] vM1(y pi/2)[b] G, G factors in x and y and a Cartesian
// column carries no rotation, so c_k EC_{6+b}(x, y) = c_k fx(x) gy_b(y) with ONE x-profile for all 21 columns (HostConsts::
// odd_cart_*).  Its row loop sums gy_b(y) * sum_{x<16} fx(x) s_o(x, y) in f32 on the vector ALU and rebuilds accumulator
// tiles 2, 7, 8, 13, 14, 19, 20 once per batch; the tables, `colmap` and the whitening fragments are the same in every mode.
constexpr int kStreams = 7;
constexpr int kTiles = 21;        // accumulator tiles = packed output tiles (what `colmap` and the whitening fragments index):
                                  // 0-2 m | per harmonic h = k-1, 3 + 6h + 2 (LUT tile 0..2) + (0: U, 1: V)
constexpr int kAccTiles = kTiles;
constexpr int kTileCols = 16;
constexpr int kPolarSlots = 10;   // a mixed tile (LUT tile 1 of a group): slots below it are polar, the others cartesian
constexpr int kPackedCols = kTiles * kTileCols;  // 336
constexpr int kUniqueTiles = 12;  // LUT tiles per patch row: 0-2 m | 3 + 3h + {0, 1, 2}

// The UNFOLDED row form, kept for LF_MKD_POOL_F16_FP6 alone (an experiment frozen as a mode): a lane holds the 8 pixels
// x in [8q, 8q+8) of the row and per harmonic k both streams meet four LUT tiles of 16 columns:
//   P0 = EPc[0:16] | Q0 = EPs[0:16] | R = EPc[16:25], EC[0:7] | S = EPs[16:25], EC[7:9], 5 unused
// into 8 products; the m stream keeps 3 tiles.  24 accumulator tiles in the row loop (the two products of relsin[0:16]
// share one); the epilogue adds / subtracts them into 21 tiles of packed output columns:
//   0-2 m | per harmonic, base 3 + 6h: relcos[0:16] | relsin[0:16] | relcos[16:25],abscos[0:7]
//        | relsin[16:25],abssin[0:7] | abscos[7:9] in slots 9,10 | abssin[7:9] in slots 9,10
constexpr int kUnfAccTiles = 24;
constexpr int kUnfUniqueTiles = 15;

struct PcaModel {
    std::vector<float> mean, eigvals, eigvecs;  // [238], [238], [238*238] row-major
};

// Reads the reference's safetensors PCA model (mkd_ref.rs:352-391). Returns "" or an error text.
std::string load_pca_safetensors(const std::string &path, PcaModel &out);

struct HostConsts {
    // ConstantData, reference layout (kept for tests / debugging)
    std::vector<float> gradient_angle;       // [1024]      phi
    std::vector<float> embedding_polar;      // [25][1024]  EP
    std::vector<float> embedding_cartesian;  // [9][1024]   EC
    std::vector<float> mean;                 // [238]
    std::vector<float> w_t;                  // [128][238]  scaled eigenvectors, transposed

    // device layouts
    // [336] packed column -> descriptor index d (0..237); -1: unused; -2 - d: the column holds MINUS entry d
    std::vector<int16_t> colmap;
    // f32 pooling fragments for v_mfma_f32_16x16x4_f32:
    //   [row y 32][unique tile 12][half 2][lane 64][i 4] = the column's (lane & 15) half at x = 4 (lane >> 4) + i
    std::vector<float> pool_b_f32;
    // f16 hi/lo pooling fragments for v_mfma_f32_16x16x32_f16 (B[k][col], k = 8*(lane>>4)+e, e = 4 half + i):
    //   [row y 32][unique tile 12][hi|lo 2][lane 64][e 8] (uint16 bit patterns); v = hi + lo, both f16
    std::vector<uint16_t> pool_b_f16;
    // Whitening as out^T = W_T x raw with the pooling accumulators as B operand: a lane (patch p, q) holds
    // packed columns 16t + 4q + i in accumulator (t, i).  A fragments = rows of W_T, K ordered to match:
    //   f16 (16x16x32): [step 11][row tile 8][hi|lo 2][lane 64][j 8], lane = (row n = lane&15, q = lane>>4),
    //        value +-W_T[16r + n][desc(16*(2s + (j>>2)) + 4q + (j&3))], 0 for padding columns
    //   f32 (16x16x4):  [tile 21][i 4][row tile 8][lane 64] = +-W_T[16r + n][desc(16t + 4q + i)]
    std::vector<uint16_t> white_a_f16;
    std::vector<float> white_a_f32;
    // LF_MKD_POOL_F16_FP6 (the unfolded row form): its own packed order, whitening fragments and row images
    //   [row y 32][unique tile 15][hi|lo 2][lane 64][e 8], pixel 8 (lane >> 4) + e.  The hi pieces, and both pieces of the m
    // stream's three tiles, are f16 as above; for the tiles of
    // the harmonics the lo piece is replaced by the lane's operand of v_mfma_scale_f32_16x16x128_f8f6f4 that carries BOTH
    // cross terms of the split: 16 e2m3 fields (12 bytes) -- field 2e = 2048 (v - hi) / T, field 2e + 1 = hi / T for the
    // lane's pixel e -- and a word with the lane's block scale T as an E8M0 byte (tiles P0 and Q0 of a harmonic share T:
    // they meet in one instruction).
    std::vector<int16_t> colmap_unfolded;       // [336], entries >= -1
    std::vector<uint16_t> pool_b_fp6;
    std::vector<uint16_t> white_a_f16_unfolded;
    // largest |L(x) -+ L(31-x)| of a LUT column relative to the column's largest value: what the fold assumes to be zero
    float lut_parity_defect = 0.f;
    // The x-odd Cartesian kernels EC 6, 7, 8 as a product (see above), built in f64 from the grid and coefficients of the
    // LUT and rounded to f32: fx at the folded x < 16, symmetrised like the LUT, (f(x) - f(31-x)) / 2; gy_0..2(y) and a pad
    // (0).  odd_cart_defect: the largest |c_k fx(x) gy_b(y) - lut value of (EC_{6+b}, c_k)| over all 32 x 32 pixels and
    // k = 0..3, relative to the column's largest value -- what LF_MKD_POOL_F16X3's row loop assumes to be zero.
    float odd_cart_fx[16] = {};
    float odd_cart_gy[32][4] = {};
    float odd_cart_defect = 0.f;
    std::vector<float> white_bias;  // [128] = -sum_d W_T[n][d] mean[d]  (whitening.glsl subtracts the mean first)
};

// Returns "" or why the model cannot be used (never aborts: include/lf_mkd.h promises a status for every failure).
std::string build_host_consts(const PcaModel &pca, HostConsts &out);

}  // namespace lfmkd
